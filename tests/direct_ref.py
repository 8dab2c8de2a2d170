"""The direct-lighting pass (rt_render_direct; include/shirley_rt.h) restated with the CPU
oracle's building blocks: or_pixel_ray for the camera ray, or_probe_segment with the path's running draw counter
for the dielectric chain, the feature vertex, its `emitted` and its `attenuation`, or_rng_f64 for the light pick,
the area sample and the sphere draws, the estimator's arithmetic operation for operation in Python floats (IEEE
binary64, math.sqrt correctly rounded, nothing fused), and or_scene_hit_at on [0.001, 1 - 2^-20] for the shadow
ray.  The device must give these arrays bit for bit wherever the vertex albedo needs no libm function."""
import ctypes as C
import math

import numpy as np

import oracle_lib as O
from ao_ref import first_segment_draw
from raytracer import _native as N

PI = 3.141592653589793
T_MIN, T_MAX = 0.001, 1.0 - 2.0 ** -20
RECTS = {N.RT_GEOM_RECT_XY: (0, 1, 2), N.RT_GEOM_RECT_YZ: (1, 2, 0), N.RT_GEOM_RECT_XZ: (0, 2, 1)}  # d1, d2, axis


def host_lights(desc):
    """rt_scene_lights_host -> (list of rt_light, n_unlisted)."""
    n, u = C.c_int32(), C.c_int32()
    assert N.rt_lib().rt_scene_lights_host(C.byref(desc), C.byref(n), C.byref(u), None) == 0
    out = (N.rt_light * max(1, n.value))()
    assert N.rt_lib().rt_scene_lights_host(C.byref(desc), C.byref(n), C.byref(u), out) == 0
    return list(out[:n.value]), u.value


def list_lights(desc):
    """The listing rule restated: [(object index, geometry, emitter, p[6], area, colour)] and the unlisted count."""
    lights, unlisted = [], 0
    for i in range(desc.n_objects):
        o = desc.objects[i]
        m = desc.materials[o.material]
        if m.kind not in (N.RT_MAT_DIFFUSE_LIGHT, N.RT_MAT_FAIRY_LIGHT):
            continue
        t = desc.textures[m.texture]
        p = list(o.p)
        ok = t.kind == N.RT_TEX_SOLID and not o.medium and not o.transform
        if o.geometry in RECTS:
            ok = ok and p[1] - p[0] > 0.0 and p[3] - p[2] > 0.0
            area = (p[1] - p[0]) * (p[3] - p[2])
        elif o.geometry == N.RT_GEOM_SPHERE:
            ok = ok and p[3] > 0.0
            area = (4.0 * PI) * (p[3] * p[3])
        else:
            ok = False
        if ok:
            lights.append((i, o.geometry, m.kind, p, area, list(t.color)))
        else:
            unlisted += 1
    return lights, unlisted


class DirectRef:
    """emission, direct [H][W][3], and what the frame holds: misses, emitter vertices (DiffuseLight / FairyLight),
    vertices that take a light sample, those samples per light kind (geometry, emitter), back-face cuts, occluded
    and unoccluded shadow rays, sphere-sample rejections, and the vertices whose albedo texture is solid (`solid`
    [H][W]: every sample of the pixel; there the device is bit-exact whatever the libm)."""

    def __init__(self, h, w):
        self.emission = np.zeros((h, w, 3))
        self.direct = np.zeros((h, w, 3))
        self.solid = np.ones((h, w), dtype=bool)
        self.misses = self.diffuse_light = self.fairy_light = self.sampled = 0
        self.cut = self.occluded = self.unoccluded = self.sphere_rejects = self.most_attempts = 0
        self.chained = 0  # dielectric vertices followed on the way to the feature vertices
        self.kinds = {}


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def light_sample(lights, seed, pixel, s, draw, x, n, a, shadow, ref=None):
    """The header's estimator at a vertex (x, n) with attenuation a on the path's draws from `draw`;
    shadow(ray6) -> bool answers the occlusion query."""
    rng = O.lib().or_rng_f64
    nl = float(len(lights))
    k = min(int(rng(seed, pixel, s, draw) * nl), len(lights) - 1)
    draw += 1
    _, geom, emitter, p, area, colour = lights[k]
    if ref is not None:
        ref.kinds[(geom, emitter)] = ref.kinds.get((geom, emitter), 0) + 1
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
        cy = -_dot(u, w) / dist if geom == N.RT_GEOM_SPHERE else abs(w[axis]) / dist
    if not (cx > 0.0 and cy > 0.0):
        if ref is not None:
            ref.cut += 1
        return [0.0, 0.0, 0.0]
    occ = shadow(list(x) + w)
    if ref is not None:
        ref.occluded += occ
        ref.unoccluded += not occ
    if occ:
        return [0.0, 0.0, 0.0]
    le = [c * cy for c in colour] if emitter == N.RT_MAT_FAIRY_LIGHT else colour
    g = ((cx * cy) / dd) * ((area * nl) / PI)
    return [(a[c] * le[c]) * g for c in range(3)]


def oracle_direct(scene, cam, seed, s_begin, s_end, chain, osc=None, rows=None):
    osc = osc or O.OracleScene(scene)
    L, d = O.lib(), scene.desc
    lights, _ = list_lights(d)
    h, w = cam.image_height, cam.image_width
    ref = DirectRef(h, w)
    ray = O._d6()
    for py in (rows if rows is not None else range(h)):
        for px in range(w):
            pixel = py * w + px
            shadow = lambda r6: bool(osc.hit(r6, T_MIN, T_MAX, index=pixel).hit)  # noqa: E731
            for s in range(s_begin, s_end):
                L.or_pixel_ray(C.byref(cam), seed, px, py, s, ray)
                draw, attempts = first_segment_draw(cam, seed, pixel, s)
                ref.most_attempts = max(ref.most_attempts, attempts)
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
                    ref.diffuse_light += m.kind == N.RT_MAT_DIFFUSE_LIGHT
                    ref.fairy_light += m.kind == N.RT_MAT_FAIRY_LIGHT
                    if m.kind in (N.RT_MAT_LAMBERTIAN, N.RT_MAT_FAIRY_LIGHT, N.RT_MAT_DIFFUSE_LIGHT):
                        if d.textures[m.texture].kind != N.RT_TEX_SOLID:
                            ref.solid[py, px] = False
                    if m.kind in (N.RT_MAT_LAMBERTIAN, N.RT_MAT_FAIRY_LIGHT) and lights:
                        assert pr.scattered
                        ref.sampled += 1
                        dl = light_sample(lights, seed, pixel, s, draw, list(pr.point), list(pr.normal),
                                          list(pr.attenuation), shadow, ref)
                for c in range(3):
                    ref.emission[py, px, c] += em[c]
                    ref.direct[py, px, c] += dl[c]
    return ref


# ---- the scenes the direct-lighting tests share -------------------------------------------------
# (object index, geometry, emitter, area, colour) of hand_scene's listed lights, computed by hand from the
# numbers below; its four unlisted emitters follow them
HAND_LIGHTS = [
    (1, N.RT_GEOM_RECT_XY, N.RT_MAT_DIFFUSE_LIGHT, 2.0 * 1.0, (4.0, 3.0, 2.0)),
    (2, N.RT_GEOM_RECT_YZ, N.RT_MAT_FAIRY_LIGHT, 2.0 * 2.0, (1.0, 2.0, 3.0)),
    (3, N.RT_GEOM_RECT_XZ, N.RT_MAT_DIFFUSE_LIGHT, 1.5 * 1.5, (5.0, 5.0, 5.0)),
    (4, N.RT_GEOM_SPHERE, N.RT_MAT_DIFFUSE_LIGHT, (4.0 * PI) * (0.5 * 0.5), (6.0, 2.0, 1.0)),
    (5, N.RT_GEOM_SPHERE, N.RT_MAT_FAIRY_LIGHT, (4.0 * PI) * (0.375 * 0.375), (2.0, 4.0, 1.0)),
]
HAND_UNLISTED = 4


def hand_scene(extras=False, sky=None):
    """A grey floor, one rect light of each orientation, a DiffuseLight and a FairyLight sphere, then the four
    emitters the listing rule leaves out: a checker-textured rect, a RectBox, a sphere of negative radius and an
    empty rect.  extras: one Lambertian occluder sphere and a glass sphere between the camera and the lights."""
    import raytracer as rt
    from raytracer import scene as S
    solid = S.TextureLoader.solid
    b = rt.SceneBuilder()
    b.set_skybox(sky or S.SkyBox.Nothing)
    b.add(S.xz_rect(-6.0, 6.0, -6.0, 6.0, 0.0), S.Lambertian(solid(0.7, 0.7, 0.7)))
    b.add(S.xy_rect(-1.0, 1.0, 2.0, 3.0, -3.5), S.DiffuseLight(solid(4.0, 3.0, 2.0)))
    b.add(S.yz_rect(0.5, 2.5, -2.0, 0.0, -3.0), S.FairyLight(solid(1.0, 2.0, 3.0)))
    b.add(S.xz_rect(-1.0, 0.5, -1.5, 0.0, 4.0), S.DiffuseLight(solid(5.0, 5.0, 5.0)))
    b.add(S.Sphere((2.5, 1.0, -1.0), 0.5), S.DiffuseLight(solid(6.0, 2.0, 1.0)))
    b.add(S.Sphere((-1.5, 0.375, 1.0), 0.375), S.FairyLight(solid(2.0, 4.0, 1.0)))
    b.add(S.xy_rect(2.0, 3.0, 2.0, 3.0, -3.25),
          S.DiffuseLight(S.TextureLoader.checker(4.0, solid(3.0, 0.0, 0.0), solid(0.0, 0.0, 3.0))))
    b.add(S.RectBox((-3.0, 0.0, 2.0), (-2.5, 0.5, 2.5)), S.DiffuseLight(solid(2.0, 2.0, 2.0)))
    b.add(S.Sphere((3.0, 0.25, 2.0), -0.25), S.FairyLight(solid(1.0, 1.0, 4.0)))
    b.add(S.xz_rect(1.0, 1.0, 0.0, 1.0, 3.75), S.DiffuseLight(solid(9.0, 9.0, 9.0)))
    if extras:
        b.add(S.Sphere((0.25, 0.625, 0.5), 0.625), S.Lambertian(solid(0.8, 0.2, 0.2)))
        b.add(S.Sphere((-0.75, 0.5, 3.0), 0.5), S.Dielectric(1.5))
    return b


def hand_camera(width=20, height=12, aperture=None):
    import raytracer as rt
    cam = rt.CameraBuilder(width=width, aspect_ratio=(width, height), vfov=40.0, focal_length=1.0,
                           aperture=aperture).build(
        rt.CameraPosition((0.5, 2.5, 10.0), (0.0, 1.25, 0.0), (0.0, 1.0, 0.0), focus_length=10.0))
    assert (cam.image_width, cam.image_height, bool(cam.has_lens)) == (width, height, aperture is not None)
    return cam


def lambert_box():
    """box-light's geometry (scenes.rs:94-127: the ground, the sphere of radius 2, the xz_rect light at y = 3.5,
    sky NONE) with solid albedos, plus a FairyLight sphere: Lambertian surfaces and listed lights only, so
    E[rt_render(max_depth = 2)] = E[emission + direct] per pixel."""
    import raytracer as rt
    from raytracer import scene as S
    solid = S.TextureLoader.solid
    b = rt.SceneBuilder()
    b.set_skybox(S.SkyBox.Nothing)
    b.add(S.xz_rect(-30.0, 30.0, -30.0, 30.0, -0.0001), S.Lambertian(solid(0.9, 0.9, 0.9)))
    b.add(S.Sphere((0.0, 2.0, 0.0), 2.0), S.Lambertian(solid(0.4, 0.6, 0.8)))
    b.add(S.xz_rect(3.0, 5.0, 1.0, 3.0, 3.5), S.DiffuseLight(solid(4.0, 4.0, 4.0)))
    b.add(S.Sphere((3.0, 0.5, 2.5), 0.5), S.FairyLight(solid(3.0, 2.0, 1.0)))
    return b


def range_means(frames):
    """K frames of per-pixel sums (each over n samples) -> (mean, standard error) of the K frame means."""
    m = np.array([float(np.mean(f)) for f in frames])
    return float(m.mean()), float(m.std(ddof=1) / math.sqrt(len(m)))
