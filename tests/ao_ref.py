"""The ambient-occlusion pass (rt_render_ao; include/shirley_rt.h, ABI 11) restated with the CPU oracle's
building blocks: or_pixel_ray for the camera ray, or_probe_segment with the path's running draw counter for the
dielectric chain and the feature vertex, or_rng_f64 for the scatter's sphere draws and or_scene_hit_at for the
occlusion ray.  Every decision is an exact f64 test and the sums are integers, so the device must give these
arrays exactly."""
import ctypes as C
import math

import numpy as np

import oracle_lib as O
from raytracer import _native as N


def first_segment_draw(cam, seed, pixel, s):
    """The path's draw counter after the camera ray: 2 jitter draws, then two per lens-disk attempt
    (random_in_unit_disk: x, y in [-1, 1), accepted when x^2 + y^2 <= 1).  Returns (draw, attempts)."""
    if not cam.has_lens:
        return 2, 0
    draw, attempts = 2, 0
    while True:
        x = -1.0 + 2.0 * O.lib().or_rng_f64(seed, pixel, s, draw)
        y = -1.0 + 2.0 * O.lib().or_rng_f64(seed, pixel, s, draw + 1)
        draw += 2
        attempts += 1
        if x * x + y * y <= 1.0:
            return draw, attempts


def scatter_direction(seed, pixel, s, draw, normal):
    """The renderer's Lambertian scatter direction at a record with `normal`, on the path's draws from `draw`:
    r = random_in_unit_sphere (core/math.rs:32-45), w = normal + unit(r), or normal where w is near zero
    (lambertian.rs:21-37).  The arithmetic is the reference's, operation for operation."""
    rng = O.lib().or_rng_f64
    while True:
        x = -1.0 + 2.0 * rng(seed, pixel, s, draw)
        y = -1.0 + 2.0 * rng(seed, pixel, s, draw + 1)
        z = -1.0 + 2.0 * rng(seed, pixel, s, draw + 2)
        draw += 3
        if (x * x + y * y) + z * z <= 1.0:
            break
    n = math.sqrt((x * x + y * y) + z * z)
    w = [normal[0] + x / n, normal[1] + y / n, normal[2] + z / n]
    if all(abs(c) < 1e-8 for c in w):
        w = [normal[0], normal[1], normal[2]]
    return w


class AoRef:
    """sums [H][W], and what the frame holds: feature vertices (hits), how many of them are occluded, misses,
    metal and chain-exhausted dielectric vertices, the most lens-disk attempts of a sample, and at the
    Lambertian vertices how many scatter directions equal or_probe_segment's own (`lambertian`, `same`)."""

    def __init__(self, h, w):
        self.sums = np.zeros((h, w))
        self.vertices = self.occluded = self.misses = self.metal = self.exhausted = 0
        self.most_attempts = self.lambertian = self.same = 0


def oracle_ao(scene, cam, seed, s_begin, s_end, chain, radius, osc=None):
    osc = osc or O.OracleScene(scene)
    L, d = O.lib(), scene.desc
    h, w = cam.image_height, cam.image_width
    ref = AoRef(h, w)
    ray = O._d6()
    for py in range(h):
        for px in range(w):
            pixel = py * w + px
            for s in range(s_begin, s_end):
                L.or_pixel_ray(C.byref(cam), seed, px, py, s, ray)
                draw, attempts = first_segment_draw(cam, seed, pixel, s)
                ref.most_attempts = max(ref.most_attempts, attempts)
                pr = osc.probe(list(ray), seed, pixel, s, draw)
                left = chain
                while (pr.object >= 0 and d.materials[d.objects[pr.object].material].kind == N.RT_MAT_DIELECTRIC
                       and pr.scattered and left > 0):
                    left -= 1
                    draw = pr.draw
                    pr = osc.probe(list(pr.origin) + list(pr.direction), seed, pixel, s, draw)
                if pr.object < 0:  # a miss sees the sky
                    ref.misses += 1
                    ref.sums[py, px] += 1.0
                    continue
                # the feature vertex, reached with the path's draw counter `draw`
                kind = d.materials[d.objects[pr.object].material].kind
                ref.vertices += 1
                ref.metal += kind == N.RT_MAT_METAL
                ref.exhausted += kind == N.RT_MAT_DIELECTRIC
                wdir = scatter_direction(seed, pixel, s, draw, list(pr.normal))
                if kind == N.RT_MAT_LAMBERTIAN:
                    ref.lambertian += 1
                    ref.same += bool(pr.scattered) and wdir == list(pr.direction)
                t_max = radius / math.sqrt((wdir[0] * wdir[0] + wdir[1] * wdir[1]) + wdir[2] * wdir[2])
                occ = bool(osc.hit(list(pr.point) + wdir, 0.001, t_max, index=pixel).hit)
                ref.occluded += occ
                ref.sums[py, px] += 0.0 if occ else 1.0
    return ref
