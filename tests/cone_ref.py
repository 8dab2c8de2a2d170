"""Solid-angle sampling of sphere lights (rt_scene_light_sampling; include/shirley_rt.h) restated
from the header's text in Python floats (IEEE binary64, math.sqrt correctly rounded, nothing fused): the light
sample in both modes (RT_LIGHT_SAMPLE_AREA, RT_LIGHT_SAMPLE_SOLID_ANGLE) for both picks (uniform, the light grid
of tests/lightgrid_ref.py), the record rt_light_sample_at / rt_light_sample_host report for it, and rt_render_nee /
rt_render_direct with a mode on the CPU oracle's building blocks (tests/nee_ref.py, tests/direct_ref.py say which).
The library's records and the device's frames must equal these bit for bit wherever no vertex albedo needs a libm
function.  In mode AREA every function here is the earlier restatements' (tests/test_light_cone.py checks that)."""
import ctypes as C
import math

import numpy as np

import oracle_lib as O
from ao_ref import first_segment_draw
from direct_ref import PI, RECTS, T_MAX, T_MIN, DirectRef, _dot, list_lights
from lightgrid_ref import Grid
from nee_ref import NeeRef
from raytracer import _native as N

AREA, CONE = N.RT_LIGHT_SAMPLE_AREA, N.RT_LIGHT_SAMPLE_SOLID_ANGLE
CUT, INSIDE = 1, 2  # rt_light_sample.flags
NAN = float("nan")


class ConeNeeRef(NeeRef):
    """NeeRef's sums and counts, plus the light samples taken from inside a sphere light and the disk rejections."""

    def __init__(self, h, w):
        super().__init__(h, w)
        self.inside = self.disk_rejects = 0

    def counts(self):
        return super().counts() + f"; {self.inside} samples from inside a sphere, {self.disk_rejects} disk rejections"


class ConeDirectRef(DirectRef):
    def __init__(self, h, w):
        super().__init__(h, w)
        self.inside = self.disk_rejects = 0


def cone_of(c, r, x):
    """wc, dc2 and om = 1 - cos(theta_max) of the sphere (c, r) seen from x; om is None from inside or on it."""
    wc = [c[0] - x[0], c[1] - x[1], c[2] - x[2]]
    dc2 = (wc[0] * wc[0] + wc[1] * wc[1]) + wc[2] * wc[2]
    if not dc2 > r * r:
        return wc, dc2, None
    s2 = (r * r) / dc2
    cm = math.sqrt(1.0 - s2)
    return wc, dc2, s2 / (1.0 + cm)


def cone_point(c, r, x, wc, dc2, om, px, py):
    """The header's sample for the disk point (px, py) -> (w, u)."""
    dc = math.sqrt(dc2)
    a = [wc[0] / dc, wc[1] / dc, wc[2] / dc]
    sg = -1.0 if a[2] < 0.0 else 1.0
    A = -1.0 / (sg + a[2])
    B = (a[0] * a[1]) * A
    t1 = [1.0 + ((sg * a[0]) * a[0]) * A, sg * B, -(sg * a[0])]
    t2 = [B, sg + (a[1] * a[1]) * A, -a[1]]
    q = px * px + py * py
    e = q * om
    ct = 1.0 - e
    k = math.sqrt(om * (1.0 + ct))
    k1, k2 = px * k, py * k
    omega = [(t1[i] * k1 + t2[i] * k2) + a[i] * ct for i in range(3)]
    st2 = e * (1.0 + ct)
    disc = r * r - dc2 * st2
    disc = disc if disc > 0.0 else 0.0
    ds = dc * ct - math.sqrt(disc)
    w = [omega[i] * ds for i in range(3)]
    u = [((x[i] + w[i]) - c[i]) / r for i in range(3)]
    return w, u


class Sample:
    """A light sample before its shadow ray: light k, flags, the draw counter after it, w, cx, cy, and what the
    value's factor needs (d2, the pick's probability pk, the cone's om, whether the cone form applies), the cell."""


def sample_point(grid, lights, mode, seed, pixel, s, draw, x, n, ref=None):
    rng = O.lib().or_rng_f64
    out = Sample()
    nl = float(len(lights))
    if grid is not None:
        out.cell = grid.cell(x)
        k, out.pk = grid.pick(out.cell, rng(seed, pixel, s, draw))
    else:
        out.cell, out.pk = 0, 1.0
        k = min(int(rng(seed, pixel, s, draw) * nl), len(lights) - 1)
    draw += 1
    _, geom, emitter, p, area, colour = lights[k]
    out.k, out.om, out.d2 = k, 0.0, 0.0
    out.cone = mode == CONE and geom == N.RT_GEOM_SPHERE
    if ref is not None:
        ref.kinds[(geom, emitter)] = ref.kinds.get((geom, emitter), 0) + 1
    u = None
    if out.cone:
        c, r = p[0:3], p[3]
        wc, dc2, om = cone_of(c, r, x)
        if om is None:
            if ref is not None:
                ref.inside += 1
            out.flags, out.draw, out.w, out.cx, out.cy = INSIDE, draw, [0.0, 0.0, 0.0], 0.0, 0.0
            return out
        while True:
            px = -1.0 + 2.0 * rng(seed, pixel, s, draw)
            py = -1.0 + 2.0 * rng(seed, pixel, s, draw + 1)
            draw += 2
            if px * px + py * py <= 1.0:
                break
            if ref is not None:
                ref.disk_rejects += 1
        out.om = om
        w, u = cone_point(c, r, x, wc, dc2, om, px, py)
    elif geom == N.RT_GEOM_SPHERE:
        while True:
            rx = -1.0 + 2.0 * rng(seed, pixel, s, draw)
            ry = -1.0 + 2.0 * rng(seed, pixel, s, draw + 1)
            rz = -1.0 + 2.0 * rng(seed, pixel, s, draw + 2)
            draw += 3
            if (rx * rx + ry * ry) + rz * rz <= 1.0:
                break
            if ref is not None:
                ref.sphere_rejects += 1
        ln = math.sqrt((rx * rx + ry * ry) + rz * rz)
        u = [rx / ln, ry / ln, rz / ln]
        y = [p[0] + u[0] * p[3], p[1] + u[1] * p[3], p[2] + u[2] * p[3]]
        w = [y[0] - x[0], y[1] - x[1], y[2] - x[2]]
    else:
        d1, d2, axis = RECTS[geom]
        xi1 = rng(seed, pixel, s, draw)
        xi2 = rng(seed, pixel, s, draw + 1)
        draw += 2
        y = [0.0, 0.0, 0.0]
        y[d1] = p[0] + xi1 * (p[1] - p[0])
        y[d2] = p[2] + xi2 * (p[3] - p[2])
        y[axis] = p[4]
        w = [y[0] - x[0], y[1] - x[1], y[2] - x[2]]
    dd = _dot(w, w)
    dist = math.sqrt(dd)
    if dist == 0.0:  # (the device's 0 / 0 is a NaN: cut)
        cx = cy = NAN
    else:
        cx = _dot(n, w) / dist
        cy = -_dot(u, w) / dist if geom == N.RT_GEOM_SPHERE else abs(w[RECTS[geom][2]]) / dist
    out.draw, out.w, out.cx, out.cy, out.d2 = draw, w, cx, cy, dd
    out.flags = 0 if (cx > 0.0 and cy > 0.0) else CUT
    return out


def g_factor(sm, lights, mis, grid_pick):
    """The factor g of an uncut sample's value (a * Le) * g."""
    nl = float(len(lights))
    area = lights[sm.k][4]
    if sm.cone:
        if mis:
            gs = sm.cx / PI
            pl = sm.pk / ((2.0 * PI) * sm.om) if grid_pick else 1.0 / (((2.0 * PI) * sm.om) * nl)
            return gs / (pl + gs)
        return sm.cx * ((2.0 * sm.om) / sm.pk if grid_pick else (2.0 * sm.om) * nl)
    if mis:
        gs = ((sm.cx * sm.cy) / sm.d2) / PI
        pl = sm.pk / area if grid_pick else 1.0 / (area * nl)
        return gs / (pl + gs)
    return ((sm.cx * sm.cy) / sm.d2) * ((area / sm.pk if grid_pick else area * nl) / PI)


def record(grid, lights, mode, seed, i, x, n):
    """What rt_light_sample_at / rt_light_sample_host report for vertex i:
    (light, flags, draws, w[3], cx, cy, g_plain, g_mis)."""
    sm = sample_point(grid, lights, mode, seed, i, 0, 0, x, n)
    g = [0.0, 0.0] if sm.flags else [g_factor(sm, lights, mis, grid is not None) for mis in (False, True)]
    return (sm.k, sm.flags, sm.draw, sm.w[0], sm.w[1], sm.w[2], sm.cx, sm.cy, g[0], g[1])


def light_sample(grid, lights, mode, seed, pixel, s, draw, x, n, a, shadow, mis, ref=None):
    """The header's light sample at a vertex (x, n) with attenuation a on the path's draws from `draw`, grid None:
    the uniform pick -> (value, the draw counter after the sample, the vertex's cell)."""
    sm = sample_point(grid, lights, mode, seed, pixel, s, draw, x, n, ref)
    zero = [0.0, 0.0, 0.0]
    if sm.flags:
        if ref is not None and sm.flags == CUT:
            ref.cut += 1
        return zero, sm.draw, sm.cell
    occ = shadow(list(x) + sm.w)
    if ref is not None:
        ref.occluded += occ
        ref.unoccluded += not occ
    if occ:
        return zero, sm.draw, sm.cell
    _, _, emitter, _, _, colour = lights[sm.k]
    le = [c * sm.cy for c in colour] if emitter == N.RT_MAT_FAIRY_LIGHT else colour
    g = g_factor(sm, lights, mis, grid is not None)
    return [(a[c] * le[c]) * g for c in range(3)], sm.draw, sm.cell


def emission_weight(grid, lights, mode, mis, lj, cell_prev, cxp, origin, dv, normal, t):
    """ws of a listed hit on light lj (a rect, or a sphere's front face) after a vertex that took a sample."""
    _, geom, _, p, area, _ = lights[lj]
    nl = float(len(lights))
    if mode == CONE and geom == N.RT_GEOM_SPHERE:
        _, _, om = cone_of(p[0:3], p[3], origin)
        if om is None or not cxp > 0.0:
            return 1.0
        if not mis:
            return 0.0
        gs = cxp / PI
        pl = (grid.prob(cell_prev, lj) / ((2.0 * PI) * om) if grid is not None
              else 1.0 / (((2.0 * PI) * om) * nl))
        return gs / (pl + gs)
    if not mis:
        return 0.0
    ld2 = (dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]
    ld = math.sqrt(ld2)
    cy = -_dot(normal, dv) / ld
    d2 = (t * t) * ld2
    if cxp > 0.0 and cy > 0.0:
        gs = ((cxp * cy) / d2) / PI
        pl = grid.prob(cell_prev, lj) / area if grid is not None else 1.0 / (area * nl)
        return gs / (pl + gs)
    return 1.0


def oracle_nee(scene, cam, seed, s_begin, s_end, max_depth, mis, cells, mode, osc=None, stats=True):
    """rt_render_nee after rt_scene_light_pick(cells) (0: the uniform pick) and rt_scene_light_sampling(mode)."""
    osc = osc or O.OracleScene(scene)
    L, d = O.lib(), scene.desc
    lights, _ = list_lights(d)
    grid = Grid(lights, cells) if cells > 0 and lights else None
    lidx = {l[0]: j for j, l in enumerate(lights)}
    h, w = cam.image_height, cam.image_width
    ref = ConeNeeRef(h, w)
    cnt = ref if stats else None
    ray = O._d6()
    textured = (N.RT_MAT_LAMBERTIAN, N.RT_MAT_FAIRY_LIGHT, N.RT_MAT_DIFFUSE_LIGHT)
    for py in range(h):
        for px in range(w):
            pixel = py * w + px
            shadow = lambda r6: bool(osc.hit(r6, T_MIN, T_MAX, index=pixel).hit)  # noqa: E731
            for s in range(s_begin, s_end):
                if max_depth <= 0:
                    continue
                L.or_pixel_ray(C.byref(cam), seed, px, py, s, ray)
                draw, attempts = first_segment_draw(cam, seed, pixel, s)
                ref.most_attempts = max(ref.most_attempts, attempts)
                r = list(ray)
                att, rad = [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]
                prev, cxp, cell_prev = False, 0.0, 0
                k = 1
                while True:
                    ref.longest = max(ref.longest, k)
                    pr = osc.probe(r, seed, pixel, s, draw)
                    if pr.object < 0:  # the sky is never listed
                        ref.misses += 1
                        for c in range(3):
                            rad[c] += att[c] * pr.emitted[c]
                        break
                    obj = d.objects[pr.object]
                    m = d.materials[obj.material]
                    if m.kind in textured and d.textures[m.texture].kind != N.RT_TEX_SOLID:
                        ref.solid[py, px] = False
                    ref.dielectric += m.kind == N.RT_MAT_DIELECTRIC
                    if pr.emits:
                        ws = 1.0
                        if prev and pr.object in lidx:
                            if obj.geometry == N.RT_GEOM_SPHERE and not pr.front_face:
                                ref.sphere_back += 1
                            else:
                                if obj.geometry == N.RT_GEOM_SPHERE:
                                    ref.reweighted_sphere_front += 1
                                else:
                                    ref.reweighted_rect += 1
                                ws = emission_weight(grid, lights, mode, mis, lidx[pr.object], cell_prev, cxp, r[0:3],
                                                     r[3:6], list(pr.normal), pr.t)
                        for c in range(3):
                            rad[c] += (att[c] * pr.emitted[c]) * ws
                    if not pr.scattered:
                        break
                    draw = pr.draw
                    prev = False
                    a = list(pr.attenuation)
                    if m.kind in (N.RT_MAT_LAMBERTIAN, N.RT_MAT_FAIRY_LIGHT) and lights and k < max_depth:
                        if cnt is not None:
                            cnt.sampled += 1
                        dl, draw, cell_prev = light_sample(grid, lights, mode, seed, pixel, s, draw, list(pr.point),
                                                           list(pr.normal), a, shadow, mis, cnt)
                        for c in range(3):
                            rad[c] += att[c] * dl[c]
                        prev = True
                        dv = list(pr.direction)
                        cxp = _dot(list(pr.normal), dv) / math.sqrt(_dot(dv, dv))
                    for c in range(3):
                        att[c] *= a[c]
                    r = list(pr.origin) + list(pr.direction)
                    k += 1
                    if k > max_depth:
                        ref.depth_cut += 1
                        break
                for c in range(3):
                    ref.sums[py, px, c] += rad[c]
    return ref


def oracle_direct(scene, cam, seed, s_begin, s_end, chain, cells, mode, osc=None):
    """rt_render_direct after rt_scene_light_pick(cells) and rt_scene_light_sampling(mode)."""
    osc = osc or O.OracleScene(scene)
    L, d = O.lib(), scene.desc
    lights, _ = list_lights(d)
    grid = Grid(lights, cells) if cells > 0 and lights else None
    h, w = cam.image_height, cam.image_width
    ref = ConeDirectRef(h, w)
    ray = O._d6()
    for py in range(h):
        for px in range(w):
            pixel = py * w + px
            shadow = lambda r6: bool(osc.hit(r6, T_MIN, T_MAX, index=pixel).hit)  # noqa: E731
            for s in range(s_begin, s_end):
                L.or_pixel_ray(C.byref(cam), seed, px, py, s, ray)
                draw, _ = first_segment_draw(cam, seed, pixel, s)
                pr = osc.probe(list(ray), seed, pixel, s, draw)
                left = chain
                while (pr.object >= 0 and d.materials[d.objects[pr.object].material].kind == N.RT_MAT_DIELECTRIC
                       and pr.scattered and left > 0):
                    left -= 1
                    ref.chained += 1
                    draw = pr.draw
                    pr = osc.probe(list(pr.origin) + list(pr.direction), seed, pixel, s, draw)
                em = list(pr.emitted) if pr.emits else [0.0, 0.0, 0.0]
                dl = [0.0, 0.0, 0.0]
                if pr.object < 0:
                    ref.misses += 1
                else:
                    m = d.materials[d.objects[pr.object].material]
                    if m.kind in (N.RT_MAT_LAMBERTIAN, N.RT_MAT_FAIRY_LIGHT, N.RT_MAT_DIFFUSE_LIGHT):
                        if d.textures[m.texture].kind != N.RT_TEX_SOLID:
                            ref.solid[py, px] = False
                    if m.kind in (N.RT_MAT_LAMBERTIAN, N.RT_MAT_FAIRY_LIGHT) and lights:
                        ref.sampled += 1
                        dl, _, _ = light_sample(grid, lights, mode, seed, pixel, s, draw, list(pr.point),
                                                list(pr.normal), list(pr.attenuation), shadow, False, ref)
                for c in range(3):
                    ref.emission[py, px, c] += em[c]
                    ref.direct[py, px, c] += dl[c]
    return ref


# ---- the vertex set of the record tests -------------------------------------------------------------
EDGES = ("near40", "near10", "far", "inside", "centre", "surface", "az-1", "az+1", "az+0", "az-0", "away",
         "tangent+", "tangent-")


def edge_vertices(c, r):
    """(name, x, n) per entry of EDGES for the sphere light (c, r): the vertex r (1 + 2^-40) and r (1 + 2^-10) from
    the centre, 10^6 r away, inside, at the centre, on the surface (exactly, where c.y - r is exact), the basis's
    sign cases a.z = -1, +1, +0.0 and (where c.z == 0: the quotient of the least denormal rounds to it) -0.0, a
    normal facing away from every light, and the two normals tangent to the cone's edge."""
    d = 1.0
    st = r / d
    ct = math.sqrt(1.0 - st * st)
    return [
        ("near40", [c[0] + r * (1.0 + 2.0 ** -40), c[1], c[2]], [-1.0, 0.0, 0.0]),
        ("near10", [c[0], c[1] - r * (1.0 + 2.0 ** -10), c[2]], [0.0, 1.0, 0.0]),
        ("far", [c[0], c[1] - 1e6 * r, c[2]], [0.0, 1.0, 0.0]),
        ("inside", [c[0] + r * 0.5, c[1], c[2]], [0.0, 1.0, 0.0]),
        ("centre", list(c), [0.0, 1.0, 0.0]),
        ("surface", [c[0], c[1] - r, c[2]], [0.0, 1.0, 0.0]),
        ("az-1", [c[0], c[1], c[2] + 2.0], [0.0, 0.0, -1.0]),
        ("az+1", [c[0], c[1], c[2] - 2.0], [0.0, 0.0, 1.0]),
        ("az+0", [c[0] + 3.0, c[1], c[2]], [-1.0, 0.0, 0.0]),
        ("az-0", [c[0] + 3.0, c[1], c[2] + 5e-324], [-1.0, 0.0, 0.0]),
        ("away", [c[0], -1.0, c[2]], [0.0, -1.0, 0.0]),
        ("tangent+", [c[0], c[1] - d, c[2]], [ct, -st, 0.0]),
        ("tangent-", [c[0], c[1] - d, c[2]], [-ct, st, 0.0]),
    ]


def vertex_set(lights, seed, count=2000):
    """`count` vertices (points, normals, tags): slot i's uniform pick on the key (seed, pixel = i, sample 0, draw 0)
    is known, so three slots in four whose pick is a sphere light hold that light's next edge vertex (tag: its
    EDGES name) — under the uniform pick every edge vertex samples the light it was built for — and the others a
    random vertex of the box [-6, 6] x [-1, 5] x [-6, 6] with a random unit normal (tag None)."""
    rng = O.lib().or_rng_f64
    rs = np.random.RandomState(seed & 0xFFFFFFFF)
    nl = float(len(lights))
    edges = {j: edge_vertices(l[3][0:3], l[3][3]) for j, l in enumerate(lights) if l[1] == N.RT_GEOM_SPHERE}
    used = {j: 0 for j in edges}
    pts, nrm, tags = [], [], []
    for i in range(count):
        k = min(int(rng(seed, i, 0, 0) * nl), len(lights) - 1)
        if k in edges and i % 4 != 3:
            tag, x, n = edges[k][used[k] % len(edges[k])]
            used[k] += 1
        else:
            x = [float(v) for v in rs.uniform([-6.0, -1.0, -6.0], [6.0, 5.0, 6.0])]
            v = rs.normal(size=3)
            n = [float(t) for t in v / np.linalg.norm(v)]
            tag = None
        pts.append(x)
        nrm.append(n)
        tags.append(tag)
    return np.array(pts), np.array(nrm), tags


# ---- expectation ---------------------------------------------------------------------------------
def _range_job(args):
    """One sample range of expectation_figures (a process of its own builds its scene)."""
    make, M, k, n, K, seed, flags, cells, modes = args
    scene, cam = make()
    osc = O.OracleScene(scene)
    ren, _ = osc.render(cam, O.params(K * n, M, seed, chunk=K * n, sample_begin=k * n, sample_count=n), threads=1)
    out = [float(ren.mean())]
    for mode in modes:
        for mis in flags:
            out.append(float(oracle_nee(scene, cam, seed, k * n, (k + 1) * n, M, mis, cells, mode, osc,
                                        stats=False).sums.mean()))
    return out


def expectation_figures(make, max_depth, K, n, seed, cells, modes=(AREA, CONE), flags=(False, True), processes=1):
    """nee_ref.expectation_figures with a mode: frame mean per sample +- standard error over K disjoint ranges of
    n spp, of or_render_rows first, then of the restatement for each mode and, within it, each flag value."""
    jobs = [(make, max_depth, k, n, K, seed, tuple(flags), cells, tuple(modes)) for k in range(K)]
    if processes > 1:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(processes) as pool:
            rows = pool.map(_range_job, jobs)
    else:
        rows = [_range_job(j) for j in jobs]
    arr = np.array(rows) / n
    return [(float(m), float(sd / math.sqrt(K))) for m, sd in zip(arr.mean(0), arr.std(0, ddof=1))]
