"""The light-sampling path integrator (rt_render_nee; include/shirley_rt.h) restated with the CPU
oracle's building blocks: or_pixel_ray for the camera ray, or_probe_segment with the path's running draw counter
for every segment (the closest hit, the record, `emitted`, `scatter` on the renderer's own draws), or_rng_f64 for
the light sample's draws, or_scene_hit_at on [0.001, 1 - 2^-20] for the shadow ray, and the weights' arithmetic
operation for operation in Python floats (IEEE binary64, math.sqrt correctly rounded, nothing fused).  The device
must give these sums bit for bit wherever no vertex albedo of the pixel needs a libm function."""
import ctypes as C
import math

import numpy as np

import oracle_lib as O
from ao_ref import first_segment_draw
from direct_ref import PI, RECTS, T_MAX, T_MIN, _dot, list_lights
from raytracer import _native as N


class NeeRef:
    """sums [H][W][3], `solid` [H][W] (every vertex albedo of every sample of the pixel is a solid texture), and
    what the frame holds: light samples per (geometry, emitter), cuts, occluded and unoccluded shadow rays, sphere
    rejections, re-weighted hits on a rect / a front-face sphere, listed hits on a sphere's back face (never
    re-weighted), the longest path, paths cut by max_depth, misses, dielectric vertices and the most lens-disk
    attempts of a sample."""

    def __init__(self, h, w):
        self.sums = np.zeros((h, w, 3))
        self.solid = np.ones((h, w), dtype=bool)
        self.kinds = {}
        self.sampled = self.cut = self.occluded = self.unoccluded = self.sphere_rejects = 0
        self.reweighted_rect = self.reweighted_sphere_front = self.sphere_back = 0
        self.longest = self.depth_cut = self.misses = self.dielectric = self.most_attempts = 0

    @property
    def reweighted(self):
        return self.reweighted_rect + self.reweighted_sphere_front

    def counts(self):
        return (f"{self.sampled} light samples {self.kinds}, {self.cut} cut, {self.occluded} occluded, "
                f"{self.unoccluded} unoccluded, {self.sphere_rejects} sphere rejections; re-weighted hits: "
                f"{self.reweighted_rect} rect, {self.reweighted_sphere_front} front-face sphere "
                f"({self.sphere_back} back-face sphere hits left alone); longest path {self.longest}, "
                f"{self.depth_cut} paths cut by max_depth, {self.misses} misses, {self.dielectric} dielectric vertices")


def light_sample(lights, seed, pixel, s, draw, x, n, a, shadow, mis, ref=None):
    """The header's light sample at a vertex (x, n) with attenuation a on the path's draws from `draw`;
    shadow(ray6) -> bool answers the occlusion query.  Returns (value, the draw counter after the sample)."""
    rng = O.lib().or_rng_f64
    nl = float(len(lights))
    k = min(int(rng(seed, pixel, s, draw) * nl), len(lights) - 1)
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
        return [0.0, 0.0, 0.0], draw
    occ = shadow(list(x) + w)
    if ref is not None:
        ref.occluded += occ
        ref.unoccluded += not occ
    if occ:
        return [0.0, 0.0, 0.0], draw
    le = [c * cy for c in colour] if emitter == N.RT_MAT_FAIRY_LIGHT else colour
    if mis:
        gs = ((cx * cy) / dd) / PI
        pl = 1.0 / (area * nl)
        g = gs / (pl + gs)
    else:
        g = ((cx * cy) / dd) * ((area * nl) / PI)
    return [(a[c] * le[c]) * g for c in range(3)], draw


def oracle_nee(scene, cam, seed, s_begin, s_end, max_depth, mis, osc=None, stats=True):
    osc = osc or O.OracleScene(scene)
    L, d = O.lib(), scene.desc
    lights, _ = list_lights(d)
    lidx = {l[0]: j for j, l in enumerate(lights)}
    nl = float(len(lights))
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
                prev, cxp = False, 0.0
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
                                        gs = ((cxp * cy) / d2) / PI
                                        pl = 1.0 / (lights[lidx[pr.object]][4] * nl)
                                        ws = gs / (pl + gs)
                        for c in range(3):
                            rad[c] += (att[c] * pr.emitted[c]) * ws
                    if not pr.scattered:
                        break
                    draw = pr.draw
                    prev = False
                    a = list(pr.attenuation)
                    if m.kind in (N.RT_MAT_LAMBERTIAN, N.RT_MAT_FAIRY_LIGHT) and lights and k < max_depth:
                        dl, draw = light_sample(lights, seed, pixel, s, draw, list(pr.point), list(pr.normal), a,
                                                shadow, mis, cnt)
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


def _range_job(args):
    """One sample range of expectation_figures (a process of its own builds its scene)."""
    make, M, k, n, K, seed, flags = args
    scene, cam = make()
    osc = O.OracleScene(scene)
    ren, _ = osc.render(cam, O.params(K * n, M, seed, chunk=K * n, sample_begin=k * n, sample_count=n), threads=1)
    out = [float(ren.mean())]
    for mis in flags:
        out.append(float(oracle_nee(scene, cam, seed, k * n, (k + 1) * n, M, mis, osc, stats=False).sums.mean()))
    return out


def expectation_figures(make, max_depth, K, n, seed, flags=(False, True), processes=1):
    """Frame mean per sample +- standard error over K disjoint ranges of n spp, of or_render_rows and of the
    restatement for each flag value: [(mean, se)] with the render first.  make() -> (scene, camera), picklable."""
    jobs = [(make, max_depth, k, n, K, seed, tuple(flags)) for k in range(K)]
    if processes > 1:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(processes) as pool:
            rows = pool.map(_range_job, jobs)
    else:
        rows = [_range_job(j) for j in jobs]
    arr = np.array(rows) / n
    return [(float(m), float(sd / math.sqrt(K))) for m, sd in zip(arr.mean(0), arr.std(0, ddof=1))]


def box_frame(size):
    """make() of direct_ref.lambert_box() at default_camera(size, square)."""
    import direct_ref as D
    import raytracer as rt
    return D.lambert_box().finalize(0x5EED), rt.default_camera(size, "square")


def box16():
    return box_frame(16)


def box32():
    return box_frame(32)


def cornell24():
    import raytracer as rt
    return rt.SceneBuilder.builtin("cornell", 0x5EED).finalize(0x5EED), rt.cornell_camera(24)
