"""The visibility-aware light pick (rt_scene_light_visibility; include/shirley_rt.h) restated from
the header's text in Python floats (IEEE binary64, math.sqrt correctly rounded, nothing fused) on the CPU oracle
(tests/oracle_lib.py: or_rng_f64, OracleScene.hit), tests/direct_ref.py's light list and tests/lightgrid_ref.py's
grid: the rays of a (cell, light) pair, the masks, and the rows.  `visibility_rows` hands the rows to the frame
restatements of lightgrid_ref / cone_ref / rect_ref, which build their grid by name."""
import contextlib
import copy
import math

import numpy as np

import cone_ref
import lightgrid_ref as G
import oracle_lib as O
from direct_ref import RECTS, T_MAX, T_MIN, list_lights
from raytracer import _native as N

RAYS = (1, 2, 4, 8, 16, 32)


def cell_geometry(grid, c):
    """(cell_lo, size) of row c, as the header writes them."""
    nx, ny = grid.n[0], grid.n[1]
    iz, rem = divmod(c, nx * ny)
    iy, ix = divmod(rem, nx)
    idx = (ix, iy, iz)
    size = [(grid.hi[a] - grid.lo[a]) / float(grid.n[a]) for a in range(3)]
    return [grid.lo[a] + float(idx[a]) * size[a] for a in range(3)], size


def ray(grid, lights, seed, c, i, j):
    """Ray i of (cell c, light j) -> (x, w, traced): traced False where the bit is set without a ray (w is 0 from
    inside a sphere light)."""
    rng = O.lib().or_rng_f64
    clo, size = cell_geometry(grid, c)
    x = [clo[a] + rng(seed, c, i, a) * size[a] for a in range(3)]
    _, geom, _, p, _, _ = lights[j]
    if geom == N.RT_GEOM_SPHERE:
        q, r = p[:3], p[3]
        e = [x[a] - q[a] for a in range(3)]
        e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        if not e2 > r * r:
            return x, [0.0, 0.0, 0.0], False
        le = math.sqrt(e2)
        y = [q[a] + r * (e[a] / le) for a in range(3)]
    else:
        d1, d2, axis = RECTS[geom]
        xi1 = rng(seed, c, i, 4 + 2 * j)
        xi2 = rng(seed, c, i, 5 + 2 * j)
        y = [0.0, 0.0, 0.0]
        y[d1] = p[0] + xi1 * (p[1] - p[0])
        y[d2] = p[2] + xi2 * (p[3] - p[2])
        y[axis] = p[4]
    w = [y[a] - x[a] for a in range(3)]
    w2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    return x, w, bool(w2 > 0.0)


class Masks:
    """masks [cells][L] uint32 and what the report counts: rays traced, bits set, dead points."""

    def __init__(self, grid, lights, osc, rays, seed):
        assert rays in RAYS
        L = len(lights)
        n_cells = grid.n[0] * grid.n[1] * grid.n[2]
        self.masks = np.zeros((n_cells, L), dtype=np.uint32)
        self.traced = self.no_ray = 0
        for c in range(n_cells):
            for j in range(L):
                m = 0
                for i in range(rays):
                    x, w, traced = ray(grid, lights, seed, c, i, j)
                    if traced:
                        self.traced += 1
                        bit = not osc.hit(x + w, T_MIN, T_MAX).hit
                    else:
                        self.no_ray += 1
                        bit = True
                    m |= int(bit) << i
                self.masks[c, j] = m
        self.unoccluded = sum(bin(int(m)).count("1") for m in self.masks.reshape(-1))
        valid = np.bitwise_or.reduce(self.masks, axis=1)
        self.dead_points = sum(rays - bin(int(v)).count("1") for v in valid)


def rows(grid, lights, masks, rays):
    """The rows for masks [cells][L] in the plain grid `grid` (a lightgrid_ref.Grid): its weights w_j times v_j
    where the cell has a live point, its own row where it has none."""
    L = len(lights)
    field = (1 << rays) - 1
    out = []
    items = _items(lights)
    size = [(grid.hi[a] - grid.lo[a]) / float(grid.n[a]) for a in range(3)]
    diag2 = (size[0] * size[0] + size[1] * size[1]) + size[2] * size[2]
    floor_p = G.UNIFORM / float(L)
    for c in range(len(grid.rows)):
        m = [int(v) & field for v in np.asarray(masks).reshape(-1, L)[c]]
        valid = 0
        for v in m:
            valid |= v
        kc = bin(valid).count("1")
        if kc == 0:
            out.append(list(grid.rows[c]))
            continue
        clo, _ = cell_geometry(grid, c)
        nx, ny = grid.n[0], grid.n[1]
        iz, rem = divmod(c, nx * ny)
        iy, ix = divmod(rem, nx)
        idx = (ix, iy, iz)
        chi = [grid.lo[a] + float(idx[a] + 1) * size[a] for a in range(3)]
        w, W = [], 0.0
        for j, (cen, rho2, phi) in enumerate(items):
            dd = []
            for a in range(3):
                t = clo[a] - cen[a]
                t = t if t > 0.0 else 0.0
                e = cen[a] - chi[a]
                dd.append(e if e > t else t)
            D2 = (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]
            mm = rho2 + diag2
            wj = phi / (D2 if D2 > mm else mm)
            v = (float(bin(m[j]).count("1")) + 1.0) / (float(kc) + 2.0)
            w.append(wj * v)
            W = W + w[-1]
        row, acc = [], 0.0
        if W > 0.0 and W < G.INF:
            for j in range(L):
                acc = acc + (((w[j] / W) * G.WEIGHTED) + floor_p)
                row.append(acc)
        else:
            row = [float(j + 1) / float(L) for j in range(L)]
        row[L - 1] = 1.0
        out.append(row)
    return out


def _items(lights):
    """(centre, rho2, Phi) per light, as lightgrid_ref.Grid computes them."""
    items = []
    for _, geom, _, p, area, colour in lights:
        if geom == N.RT_GEOM_SPHERE:
            c, rho2 = [p[0], p[1], p[2]], p[3] * p[3]
        else:
            d1, d2, axis = RECTS[geom]
            h1, h2 = (p[1] - p[0]) * 0.5, (p[3] - p[2]) * 0.5
            c = [0.0] * 3
            c[d1], c[d2], c[axis] = p[0] + h1, p[2] + h2, p[4]
            rho2 = h1 * h1 + h2 * h2
        s = (colour[0] + colour[1]) + colour[2]
        items.append((c, rho2, area * (s if s > 0.0 else 0.0)))
    return items


def grid_with(grid, new_rows):
    g = copy.copy(grid)
    g.rows = [list(r) for r in new_rows]
    return g


def visibility_grid(desc, cells, masks, rays):
    """lightgrid_ref.Grid of the description with the visibility rows in place of its own."""
    lights, _ = list_lights(desc)
    grid = G.Grid(lights, cells)
    return grid_with(grid, rows(grid, lights, masks, rays))


@contextlib.contextmanager
def visibility_rows(grid):
    """While it lasts, the frame restatements (lightgrid_ref.oracle_nee / oracle_direct, cone_ref's and through
    them rect_ref's) take `grid` wherever they build Grid(lights, cells)."""
    saved = G.Grid, cone_ref.Grid
    G.Grid = cone_ref.Grid = lambda lights, cells: grid
    try:
        yield grid
    finally:
        G.Grid, cone_ref.Grid = saved
