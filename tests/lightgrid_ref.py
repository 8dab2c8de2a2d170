"""The spatially weighted light pick (rt_scene_light_pick; include/shirley_rt.h) restated from the
header's text in Python floats (IEEE binary64, nothing fused): the light grid's build, the cell of a vertex, the
one-draw pick and its probability, and rt_render_direct / rt_render_nee with that pick on the CPU oracle's
building blocks (tests/direct_ref.py, tests/nee_ref.py say which).  The library's table and the device's frames
must equal these bit for bit wherever no vertex albedo needs a libm function."""
import bisect
import ctypes as C
import math

import numpy as np

import oracle_lib as O
from ao_ref import first_segment_draw
from direct_ref import PI, RECTS, T_MAX, T_MIN, DirectRef, _dot, list_lights
from nee_ref import NeeRef
from raytracer import _native as N

WEIGHTED, UNIFORM = 0.875, 0.125  # the header's two shares of a row
MAX_ENTRIES = 1 << 22
INF = float("inf")


class Grid:
    """n[3], lo[3], hi[3], n_lights and rows[(iz * n[1] + iy) * n[0] + ix] = the cell's L running sums."""

    def __init__(self, lights, cells):
        assert 1 <= cells <= 64
        L = self.n_lights = len(lights)
        self.n, self.lo, self.hi, self.rows, self.too_large = [0, 0, 0], [0.0] * 3, [0.0] * 3, [], False
        if L == 0:
            return
        items = []
        for j, (_, geom, _, p, area, colour) in enumerate(lights):
            if geom == N.RT_GEOM_SPHERE:
                r = p[3]
                c = [p[0], p[1], p[2]]
                lo = [p[a] - r for a in range(3)]
                hi = [p[a] + r for a in range(3)]
                rho2 = r * r
            else:
                d1, d2, axis = RECTS[geom]
                h1, h2 = (p[1] - p[0]) * 0.5, (p[3] - p[2]) * 0.5
                c, lo, hi = [0.0] * 3, [0.0] * 3, [0.0] * 3
                lo[d1], hi[d1], c[d1] = p[0], p[1], p[0] + h1
                lo[d2], hi[d2], c[d2] = p[2], p[3], p[2] + h2
                lo[axis] = hi[axis] = c[axis] = p[4]
                rho2 = h1 * h1 + h2 * h2
            s = (colour[0] + colour[1]) + colour[2]
            phi = area * (s if s > 0.0 else 0.0)
            items.append((c, rho2, phi))
            for a in range(3):
                self.lo[a] = lo[a] if (j == 0 or lo[a] < self.lo[a]) else self.lo[a]
                self.hi[a] = hi[a] if (j == 0 or hi[a] > self.hi[a]) else self.hi[a]
        ext = [self.hi[a] - self.lo[a] for a in range(3)]
        ext_max = ext[0]
        for a in (1, 2):
            ext_max = ext[a] if ext[a] > ext_max else ext_max
        size = [0.0] * 3
        for a in range(3):
            if not ext[a] > 0.0:
                self.n[a] = 1
            else:
                f = float(cells) * (ext[a] / ext_max)
                self.n[a] = 1 + int(f) if f < float(cells) else cells
            size[a] = ext[a] / float(self.n[a])
        self.too_large = self.n[0] * self.n[1] * self.n[2] * L > MAX_ENTRIES
        if self.too_large:
            return
        diag2 = (size[0] * size[0] + size[1] * size[1]) + size[2] * size[2]
        floor_p = UNIFORM / float(L)
        for iz in range(self.n[2]):
            for iy in range(self.n[1]):
                for ix in range(self.n[0]):
                    idx = (ix, iy, iz)
                    clo = [self.lo[a] + float(idx[a]) * size[a] for a in range(3)]
                    chi = [self.lo[a] + float(idx[a] + 1) * size[a] for a in range(3)]
                    w, W = [], 0.0
                    for c, rho2, phi in items:
                        dd = []
                        for a in range(3):
                            t = clo[a] - c[a]
                            t = t if t > 0.0 else 0.0
                            e = c[a] - chi[a]
                            dd.append(e if e > t else t)
                        D2 = (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]
                        m = rho2 + diag2
                        w.append(phi / (D2 if D2 > m else m))
                        W = W + w[-1]
                    row, acc = [], 0.0
                    if W > 0.0 and W < INF:
                        for j in range(L):
                            acc = acc + (((w[j] / W) * WEIGHTED) + floor_p)
                            row.append(acc)
                    else:
                        row = [float(j + 1) / float(L) for j in range(L)]
                    row[L - 1] = 1.0
                    self.rows.append(row)
        self.inv = [0.0 if self.n[a] == 1 else float(self.n[a]) / (self.hi[a] - self.lo[a]) for a in range(3)]

    def cdf(self):
        """[n[2]][n[1]][n[0]][L], the layout of rt_light_grid_host."""
        return np.array(self.rows, dtype=np.float64).reshape(self.n[2], self.n[1], self.n[0], self.n_lights)

    def cell(self, x):
        i = []
        for a in range(3):
            q = (x[a] - self.lo[a]) * self.inv[a]
            i.append(0 if not q >= 0.0 else self.n[a] - 1 if q >= float(self.n[a]) else int(q))
        return (i[2] * self.n[1] + i[1]) * self.n[0] + i[0]

    def prob(self, cell, j):
        row = self.rows[cell]
        return row[j] - (row[j - 1] if j else 0.0)

    def pick(self, cell, xi):
        """The smallest k with xi < cdf[k] (L - 1 if there is none) and its probability."""
        row = self.rows[cell]
        k = self.n_lights - 1 if xi != xi else min(bisect.bisect_right(row, xi), self.n_lights - 1)
        return k, self.prob(cell, k)


def grid_of(desc, cells):
    return Grid(list_lights(desc)[0], cells)


def light_sample(grid, lights, seed, pixel, s, draw, x, n, a, shadow, mis, ref=None):
    """The header's light sample with the grid pick at a vertex (x, n) with attenuation a on the path's draws
    from `draw` -> (value, the draw counter after the sample, the vertex's cell)."""
    rng = O.lib().or_rng_f64
    cell = grid.cell(x)
    k, pk = grid.pick(cell, rng(seed, pixel, s, draw))
    draw += 1
    _, geom, emitter, p, area, colour = lights[k]
    if ref is not None:
        ref.sampled += 1
        ref.kinds[(geom, emitter)] = ref.kinds.get((geom, emitter), 0) + 1
    u = None
    if geom == N.RT_GEOM_SPHERE:
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
        cx = cy = float("nan")
    else:
        cx = _dot(n, w) / dist
        cy = -_dot(u, w) / dist if geom == N.RT_GEOM_SPHERE else abs(w[RECTS[geom][2]]) / dist
    if not (cx > 0.0 and cy > 0.0):
        if ref is not None:
            ref.cut += 1
        return [0.0, 0.0, 0.0], draw, cell
    occ = shadow(list(x) + w)
    if ref is not None:
        ref.occluded += occ
        ref.unoccluded += not occ
    if occ:
        return [0.0, 0.0, 0.0], draw, cell
    le = [c * cy for c in colour] if emitter == N.RT_MAT_FAIRY_LIGHT else colour
    if mis:
        gs = ((cx * cy) / dd) / PI
        pl = pk / area
        g = gs / (pl + gs)
    else:
        g = ((cx * cy) / dd) * ((area / pk) / PI)
    return [(a[c] * le[c]) * g for c in range(3)], draw, cell


def oracle_nee(scene, cam, seed, s_begin, s_end, max_depth, mis, cells, osc=None, stats=True):
    """nee_ref.oracle_nee with the grid pick: rt_render_nee after rt_scene_light_pick(cells)."""
    osc = osc or O.OracleScene(scene)
    L, d = O.lib(), scene.desc
    lights, _ = list_lights(d)
    grid = Grid(lights, cells)
    lidx = {l[0]: j for j, l in enumerate(lights)}
    h, w = cam.image_height, cam.image_width
    ref = NeeRef(h, w)
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
                                if not mis:
                                    ws = 0.0
                                else:
                                    dv = r[3:6]
                                    ld2 = (dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]
                                    ld = math.sqrt(ld2)
                                    cy = -_dot(list(pr.normal), dv) / ld
                                    d2 = (pr.t * pr.t) * ld2
                                    if cxp > 0.0 and cy > 0.0:
                                        lj = lidx[pr.object]
                                        gs = ((cxp * cy) / d2) / PI
                                        pl = grid.prob(cell_prev, lj) / lights[lj][4]
                                        ws = gs / (pl + gs)
                        for c in range(3):
                            rad[c] += (att[c] * pr.emitted[c]) * ws
                    if not pr.scattered:
                        break
                    draw = pr.draw
                    prev = False
                    a = list(pr.attenuation)
                    if m.kind in (N.RT_MAT_LAMBERTIAN, N.RT_MAT_FAIRY_LIGHT) and lights and k < max_depth:
                        dl, draw, cell_prev = light_sample(grid, lights, seed, pixel, s, draw, list(pr.point),
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


def oracle_direct(scene, cam, seed, s_begin, s_end, chain, cells, osc=None):
    """direct_ref.oracle_direct with the grid pick: rt_render_direct after rt_scene_light_pick(cells)."""
    osc = osc or O.OracleScene(scene)
    L, d = O.lib(), scene.desc
    lights, _ = list_lights(d)
    grid = Grid(lights, cells)
    h, w = cam.image_height, cam.image_width
    ref = DirectRef(h, w)
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
                        dl, _, _ = light_sample(grid, lights, seed, pixel, s, draw, list(pr.point), list(pr.normal),
                                                list(pr.attenuation), shadow, False, ref)
                for c in range(3):
                    ref.emission[py, px, c] += em[c]
                    ref.direct[py, px, c] += dl[c]
    return ref


# ---- expectation ---------------------------------------------------------------------------------
LAMPS = [  # (x, z, radius, colour): a 3 x 3 field at y = 1.5; colour sums 1.5 ... 15
    (-3.0, -3.0, 0.15, (0.5, 0.5, 0.5)), (0.0, -3.0, 0.25, (2.0, 1.5, 1.0)), (3.0, -3.0, 0.4, (5.0, 5.0, 5.0)),
    (-3.0, 0.0, 0.3, (1.0, 2.0, 3.0)), (0.0, 0.0, 0.2, (4.0, 4.0, 2.0)), (3.0, 0.0, 0.15, (0.5, 1.0, 0.5)),
    (-3.0, 3.0, 0.4, (3.0, 1.0, 0.5)), (0.0, 3.0, 0.35, (1.0, 1.0, 1.0)), (3.0, 3.0, 0.25, (2.0, 3.0, 4.0)),
]


def lamp_field():
    """A 12 x 12 Lambertian floor, nine DiffuseLight spheres of radius 0.15 ... 0.4 at y = 1.5 whose colour sums
    differ by 10x, and two Lambertian occluder spheres at least 1 away from every lamp; solid albedos, sky NONE:
    every emitter is listed."""
    import raytracer as rt
    from raytracer import scene as S
    solid = S.TextureLoader.solid
    b = rt.SceneBuilder()
    b.set_skybox(S.SkyBox.Nothing)
    b.add(S.xz_rect(-6.0, 6.0, -6.0, 6.0, 0.0), S.Lambertian(solid(0.7, 0.7, 0.7)))
    for x, z, r, col in LAMPS:
        b.add(S.Sphere((x, 1.5, z), r), S.DiffuseLight(solid(*col)))
    b.add(S.Sphere((-1.5, 0.5, -1.5), 0.5), S.Lambertian(solid(0.8, 0.3, 0.3)))  # sqrt(4.5 + 1) - 0.5 - 0.4 > 1
    b.add(S.Sphere((1.5, 0.4, 1.5), 0.4), S.Lambertian(solid(0.3, 0.3, 0.8)))
    return b


def lamp_camera(size=32):
    import raytracer as rt
    cam = rt.CameraBuilder(width=size, aspect_ratio=(1, 1), vfov=40.0, focal_length=1.0, aperture=None).build(
        rt.CameraPosition((0.0, 7.0, 14.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), focus_length=10.0))
    assert (cam.image_width, cam.image_height) == (size, size)
    return cam


def lamp32():
    return lamp_field().finalize(0x5EED), lamp_camera(32)


def _range_job(args):
    """One sample range of expectation_figures (a process of its own builds its scene)."""
    make, M, k, n, K, seed, flags, cells = args
    scene, cam = make()
    osc = O.OracleScene(scene)
    ren, _ = osc.render(cam, O.params(K * n, M, seed, chunk=K * n, sample_begin=k * n, sample_count=n), threads=1)
    out = [float(ren.mean())]
    for mis in flags:
        out.append(float(oracle_nee(scene, cam, seed, k * n, (k + 1) * n, M, mis, cells, osc, stats=False).sums.mean()))
    return out


def expectation_figures(make, max_depth, K, n, seed, cells, flags=(False, True), processes=1):
    """nee_ref.expectation_figures for the grid pick: frame mean per sample +- standard error over K disjoint
    ranges of n spp, of or_render_rows and of the restatement for each flag value."""
    jobs = [(make, max_depth, k, n, K, seed, tuple(flags), cells) for k in range(K)]
    if processes > 1:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(processes) as pool:
            rows = pool.map(_range_job, jobs)
    else:
        rows = [_range_job(j) for j in jobs]
    arr = np.array(rows) / n
    return [(float(m), float(sd / math.sqrt(K))) for m, sd in zip(arr.mean(0), arr.std(0, ddof=1))]
