"""Render path: the MI355X replacement of render_scene's scanline loop (reference: src/main.rs:65-130,
src/raytracer/render.rs:17-70), driven through the C ABI of include/shirley_rt.h.

There is no CPU fallback: without a GPU, ``Device()`` raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native as N
from .scene import Scene


def _check(ctx, code):
    if code != 0:
        raise N.RtError(code, N.rt_lib().rt_last_error(ctx).decode())


@dataclass
class RenderSettings:
    """RenderSettings (argparse.rs:106-123) + the seed/tiling the reference lacks."""
    samples: int = 100
    max_reflect: int = 50
    seed: int = 0x5EED
    sample_chunk: int = 0
    tile_rank: int = 0
    tile_world: int = 1
    engine: str = "auto"   # auto | megakernel | wavefront | split
    timing: bool = False   # per-launch HIP-event timing of the wavefront kernels (rt_counters *_ms)
    # ABI 6: samples [sample_begin, sample_begin + sample_count) of the frame (0 = to `samples`)
    sample_begin: int = 0
    sample_count: int = 0
    partition: str = "auto"  # multi-GPU: auto | tiles | samples
    scratch_mb: int = 0      # partial-sum scratch bound per call in MiB (0 = the library default)

    ENGINES = {"auto": N.RT_ENGINE_AUTO, "megakernel": N.RT_ENGINE_MEGAKERNEL, "wavefront": N.RT_ENGINE_WAVEFRONT,
               "split": N.RT_ENGINE_SPLIT}
    PARTITIONS = {"auto": N.RT_PARTITION_AUTO, "tiles": N.RT_PARTITION_TILES, "samples": N.RT_PARTITION_SAMPLES}

    def params(self) -> N.rt_render_params:
        p = N.rt_render_params()
        p.samples, p.max_depth, p.seed = int(self.samples), int(self.max_reflect), int(self.seed)
        p.tile_rank, p.tile_world, p.sample_chunk = int(self.tile_rank), int(self.tile_world), int(self.sample_chunk)
        p.engine = self.ENGINES[self.engine] | (N.RT_ENGINE_TIMING if self.timing else 0)
        p.sample_begin, p.sample_count = int(self.sample_begin), int(self.sample_count)
        p.partition, p.scratch_mb = self.PARTITIONS[self.partition], int(self.scratch_mb)
        return p


@dataclass
class AdaptiveSettings:
    """rt_adaptive_params: every pixel gets `min_samples`, then steps of `step` samples go to the 8x8 tiles
    whose error is still above `threshold` (0 = never stop, inf = stop at min_samples), up to the
    RenderSettings' samples.  All three sample counts are multiples of the batch (sample_chunk, 0 = 4)."""
    threshold: float = 0.05
    min_samples: int = 16
    step: int = 16
    noise_floor: float = 0.01

    def params(self) -> N.rt_adaptive_params:
        a = N.rt_adaptive_params()
        a.min_samples, a.step = int(self.min_samples), int(self.step)
        a.threshold, a.noise_floor = float(self.threshold), float(self.noise_floor)
        return a


@dataclass
class DenoiseSettings:
    """rt_denoise_params with the documented defaults (include/shirley_rt.h)."""
    iterations: int = 3
    normal_power_log2: int = 4
    sigma_z: float = 0.05
    sigma_a: float = 0.2
    sigma_c: float = 2.0
    albedo_floor: float = 1e-3

    def params(self) -> N.rt_denoise_params:
        p = N.rt_denoise_params()
        p.iterations, p.normal_power_log2 = int(self.iterations), int(self.normal_power_log2)
        p.sigma_z, p.sigma_a, p.sigma_c = float(self.sigma_z), float(self.sigma_a), float(self.sigma_c)
        p.albedo_floor = float(self.albedo_floor)
        return p


def _denoise_inputs(width, height, accum_ptr, albedo_ptr, normal_ptr, depth_ptr, samples, feature_samples,
                    counts_ptr=0, variance_ptr=0) -> N.rt_denoise_inputs:
    i = N.rt_denoise_inputs()
    i.width, i.height, i.samples, i.feature_samples = int(width), int(height), int(samples), int(feature_samples)
    i.accum, i.albedo, i.normal, i.depth = accum_ptr or None, albedo_ptr or None, normal_ptr or None, depth_ptr or None
    i.counts, i.variance = counts_ptr or None, variance_ptr or None
    return i


def denoise(accum: np.ndarray, albedo: np.ndarray, normal: np.ndarray, depth: np.ndarray, samples: int = 0,
            feature_samples: int = 0, settings: Optional[DenoiseSettings] = None,
            counts: Optional[np.ndarray] = None, variance: Optional[np.ndarray] = None) -> np.ndarray:
    """rt_denoise on the host (no device): the à-trous filter on [H][W][3] sums `accum`, guided by the feature
    sums (Device.render_features over `feature_samples` samples, default: `samples`) -> filtered [H][W][3]
    sums on accum's scale.  `counts` [H][W] replaces the scalar `samples` for an adaptive frame; `variance`
    [H][W] (the variance of each pixel's mean r+g+b, moments_variance) turns the colour term on."""
    h, w, _ = accum.shape
    f64 = lambda a, shape: np.ascontiguousarray(a, dtype=np.float64).reshape(shape)  # noqa: E731
    a, al, no, de = f64(accum, (h, w, 3)), f64(albedo, (h, w, 3)), f64(normal, (h, w, 3)), f64(depth, (h, w))
    cn = None if counts is None else np.ascontiguousarray(counts, dtype=np.int32).reshape(h, w)
    va = None if variance is None else f64(variance, (h, w))
    out = np.zeros((h, w, 3), dtype=np.float64)
    i = _denoise_inputs(w, h, a.ctypes.data, al.ctypes.data, no.ctypes.data, de.ctypes.data, samples,
                        feature_samples or samples, 0 if cn is None else cn.ctypes.data,
                        0 if va is None else va.ctypes.data)
    p = (settings or DenoiseSettings()).params()
    code = N.rt_lib().rt_denoise(C.byref(i), C.byref(p), out.ctypes.data)
    if code:
        raise N.RtError(code, "rt_denoise: invalid argument")
    return out


def moments_variance(moments: np.ndarray, counts: np.ndarray, batch: int) -> np.ndarray:
    """rt_moments_variance: render_adaptive's moments and counts -> [H][W] variance of each pixel's mean r+g+b
    (`batch`: the frame's sample_chunk, 0 = 4)."""
    h, w = counts.shape
    m = np.ascontiguousarray(moments, dtype=np.float64).reshape(h, w, 2)
    n = np.ascontiguousarray(counts, dtype=np.int32)
    out = np.zeros((h, w), dtype=np.float64)
    code = N.rt_lib().rt_moments_variance(m.ctypes.data, n.ctypes.data, int(batch) or 4, w, h, out.ctypes.data)
    if code:
        raise N.RtError(code, "rt_moments_variance: invalid argument")
    return out


class Device:
    """One rt_ctx (one MI355X)."""

    def __init__(self, device: int = 0):
        lib = N.rt_lib()
        h = C.c_void_p()
        code = lib.rt_create(int(device), C.byref(h))
        if code != 0:
            raise N.RtError(code, f"rt_create(device={device}) failed: no usable HIP device")
        self._h = h
        self.scene: Optional[Scene] = None

    def close(self):
        if getattr(self, "_h", None):
            N.rt_lib().rt_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def handle(self):
        return self._h

    def upload(self, scene: Scene, bvh: str = "reference", nodes: str = "auto") -> "Device":
        """rt_scene_upload; `nodes` = auto | global | half-lds | lds (BVH node placement, tests/tuning)."""
        builder = {"reference": N.RT_BVH_REFERENCE, "sah": N.RT_BVH_SAH}[bvh]
        builder |= {"auto": 0, "global": N.RT_BVH_NODES_GLOBAL, "half-lds": N.RT_BVH_NODES_HALF_LDS,
                    "lds": N.RT_BVH_NODES_LDS}[nodes]
        _check(self._h, N.rt_lib().rt_scene_upload(self._h, scene.desc_ptr, builder))
        self.scene = scene
        return self

    def digest(self) -> int:
        """rt_scene_digest: 64-bit digest of the uploaded scene (the multi-GPU calls compare them)."""
        d = C.c_uint64()
        _check(self._h, N.rt_lib().rt_scene_digest(self._h, C.byref(d)))
        return d.value

    def stats(self) -> N.rt_scene_stats:
        s = N.rt_scene_stats()
        _check(self._h, N.rt_lib().rt_scene_stats_get(self._h, C.byref(s)))
        return s

    def hop_instance(self) -> int:
        """rt_scene_hop_instance: the megakernel instance of the uploaded scene's hop pass (0 .. 4)."""
        k = C.c_int32()
        _check(self._h, N.rt_lib().rt_scene_hop_instance(self._h, C.byref(k)))
        return k.value

    def render(self, camera: N.rt_camera, settings: RenderSettings) -> np.ndarray:
        """Whole frame -> [H][W][3] f64 per-pixel sums, row 0 = bottom (Image.data layout)."""
        out = np.zeros((camera.image_height, camera.image_width, 3), dtype=np.float64)
        p = settings.params()
        _check(self._h, N.rt_lib().rt_render(self._h, C.byref(camera), C.byref(p), out.ctypes.data))
        return out

    def render_adaptive(self, camera: N.rt_camera, settings: RenderSettings, adaptive: AdaptiveSettings):
        """rt_render_adaptive -> (accum [H][W][3] sums over each pixel's own samples, counts [H][W] int32,
        moments [H][W][2] (m1, m2 of the batch sums' r+g+b), tile_error [tiles_y][tiles_x], report)."""
        h, w = camera.image_height, camera.image_width
        accum = np.zeros((h, w, 3), dtype=np.float64)
        counts = np.zeros((h, w), dtype=np.int32)
        moments = np.zeros((h, w, 2), dtype=np.float64)
        tile_error = np.zeros(((h + 7) // 8, (w + 7) // 8), dtype=np.float64)
        report = N.rt_adaptive_report()
        p, a = settings.params(), adaptive.params()
        _check(self._h, N.rt_lib().rt_render_adaptive(self._h, C.byref(camera), C.byref(p), C.byref(a),
                                                      accum.ctypes.data, counts.ctypes.data, moments.ctypes.data,
                                                      tile_error.ctypes.data, C.byref(report)))
        return accum, counts, moments, tile_error, report

    def render_features(self, camera: N.rt_camera, settings: RenderSettings, chain: int = 8):
        """rt_render_features -> (albedo [H][W][3], normal [H][W][3], depth [H][W]) f64 sums over the settings'
        sample range, row 0 = bottom; `chain`: dielectric vertices a sample's path is followed through."""
        h, w = camera.image_height, camera.image_width
        albedo = np.zeros((h, w, 3), dtype=np.float64)
        normal = np.zeros((h, w, 3), dtype=np.float64)
        depth = np.zeros((h, w), dtype=np.float64)
        p = settings.params()
        _check(self._h, N.rt_lib().rt_render_features(self._h, C.byref(camera), C.byref(p), int(chain),
                                                      albedo.ctypes.data, normal.ctypes.data, depth.ctypes.data))
        return albedo, normal, depth

    def render_features_device(self, camera, settings: RenderSettings, chain: int, albedo_ptr: int, normal_ptr: int,
                               depth_ptr: int, stream: int = 0):
        """rt_render_features_device: device [H][W][3], [H][W][3], [H][W] f64 outputs (a pointer may be 0)."""
        p = settings.params()
        _check(self._h, N.rt_lib().rt_render_features_device(
            self._h, C.byref(camera), C.byref(p), int(chain), C.c_void_p(albedo_ptr or None),
            C.c_void_p(normal_ptr or None), C.c_void_p(depth_ptr or None), C.c_void_p(stream or None)))

    def denoise_device(self, width: int, height: int, accum_ptr: int, albedo_ptr: int, normal_ptr: int,
                       depth_ptr: int, out_ptr: int, samples: int = 0, feature_samples: int = 0,
                       settings: Optional[DenoiseSettings] = None, counts_ptr: int = 0, variance_ptr: int = 0,
                       stream: int = 0):
        """rt_denoise_device: `denoise` on device buffers, asynchronous on `stream`; bit-identical to the host's."""
        i = _denoise_inputs(width, height, accum_ptr, albedo_ptr, normal_ptr, depth_ptr, samples,
                            feature_samples or samples, counts_ptr, variance_ptr)
        p = (settings or DenoiseSettings()).params()
        _check(self._h, N.rt_lib().rt_denoise_device(self._h, C.byref(i), C.byref(p), C.c_void_p(out_ptr or None),
                                                     C.c_void_p(stream or None)))

    def moments_variance_device(self, moments_ptr: int, counts_ptr: int, batch: int, width: int, height: int,
                                out_ptr: int, stream: int = 0):
        """rt_moments_variance_device: `moments_variance` on device buffers."""
        _check(self._h, N.rt_lib().rt_moments_variance_device(
            self._h, C.c_void_p(moments_ptr or None), C.c_void_p(counts_ptr or None), int(batch) or 4, int(width),
            int(height), C.c_void_p(out_ptr or None), C.c_void_p(stream or None)))

    def tonemap_counts_device(self, accum_ptr: int, counts_ptr: int, width: int, height: int, rgb8_ptr: int,
                              stream: int = 0):
        """rt_tonemap_counts_device: as tonemap_device with a device [H][W] int32 image of per-pixel counts."""
        _check(self._h, N.rt_lib().rt_tonemap_counts_device(self._h, C.c_void_p(accum_ptr), C.c_void_p(counts_ptr),
                                                            int(width), int(height), C.c_void_p(rgb8_ptr),
                                                            C.c_void_p(stream or None)))

    def render_scanlines(self, camera: N.rt_camera, settings: RenderSettings, line_begin: int,
                         line_end: int) -> np.ndarray:
        out = np.zeros((max(0, line_end - line_begin), camera.image_width, 3), dtype=np.float64)
        p = settings.params()
        _check(self._h, N.rt_lib().rt_render_scanlines(self._h, C.byref(camera), C.byref(p), line_begin, line_end,
                                                       out.ctypes.data))
        return out

    def render_device(self, camera, settings: RenderSettings, accum_ptr: int, stream: int = 0):
        p = settings.params()
        _check(self._h, N.rt_lib().rt_render_device(self._h, C.byref(camera), C.byref(p), C.c_void_p(accum_ptr),
                                                    C.c_void_p(stream or None)))

    def render_tiles_device(self, camera, settings: RenderSettings, packed_ptr: int, stream: int = 0):
        p = settings.params()
        _check(self._h, N.rt_lib().rt_render_tiles_device(self._h, C.byref(camera), C.byref(p),
                                                          C.c_void_p(packed_ptr), C.c_void_p(stream or None)))

    def unpack_tiles_device(self, camera, world: int, gathered_ptr: int, accum_ptr: int, stream: int = 0):
        _check(self._h, N.rt_lib().rt_unpack_tiles_device(self._h, C.byref(camera), int(world),
                                                          C.c_void_p(gathered_ptr), C.c_void_p(accum_ptr),
                                                          C.c_void_p(stream or None)))

    def tonemap_device(self, accum_ptr: int, width: int, height: int, samples: int, rgb8_ptr: int,
                       stream: int = 0):
        """rt_tonemap_device: device [H][W][3] f64 sums -> device RGB8, row 0 = top (to_image)."""
        _check(self._h, N.rt_lib().rt_tonemap_device(self._h, C.c_void_p(accum_ptr), int(width), int(height),
                                                     int(samples), C.c_void_p(rgb8_ptr), C.c_void_p(stream or None)))

    def hit(self, rays: np.ndarray, t_min: float = 0.001, t_max: float = float("inf"), traversal: str = "binary"):
        """Closest hits for rays [n][6] (Hittable for Scene, scene/mod.rs:180-190) -> rt_hit array.
        traversal: "binary" (the 2-wide f64 tree, rt_scene_hit) or "render" (the 4-wide f32-inflated
        traversal the trace kernel runs, rt_scene_hit_ex(RT_TRAVERSAL_RENDER))."""
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        out = (N.rt_hit * max(1, len(r)))()
        if traversal == "binary":
            code = N.rt_lib().rt_scene_hit(self._h, r.ctypes.data, len(r), float(t_min), float(t_max), out)
        else:
            tv = {"render": N.RT_TRAVERSAL_RENDER}[traversal]
            code = N.rt_lib().rt_scene_hit_ex(self._h, r.ctypes.data, len(r), float(t_min), float(t_max), tv, out)
        _check(self._h, code)
        return out[:len(r)]

    def occluded(self, rays: np.ndarray, t_min: float = 0.001, t_max=float("inf")) -> np.ndarray:
        """rt_scene_occluded for rays [n][6] -> uint8 [n]: 1 where some object is hit with t in [t_min, t_max]
        (exactly where hit(..., traversal="render") reports an object).  `t_max`: a float, or an array [n] of
        per-ray bounds (a shadow ray's distance to its light)."""
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        each = None
        if np.ndim(t_max) > 0:
            each = np.ascontiguousarray(t_max, dtype=np.float64).reshape(-1)
            if len(each) != len(r):
                raise ValueError("t_max array must hold one bound per ray")
        out = np.zeros(max(1, len(r)), dtype=np.uint8)
        _check(self._h, N.rt_lib().rt_scene_occluded(
            self._h, r.ctypes.data if len(r) else out.ctypes.data, len(r), float(t_min),
            float("inf") if each is not None else float(t_max),
            each.ctypes.data if each is not None and len(r) else None, out.ctypes.data))
        return out[:len(r)]

    def occluded_device(self, rays_ptr: int, n: int, out_ptr: int, t_min: float = 0.001, t_max: float = float("inf"),
                        t_max_each_ptr: int = 0, stream: int = 0):
        """rt_scene_occluded_device: device rays [n][6] f64, optional device bounds [n] f64 (0: `t_max` for
        every ray) -> device uint8 [n]; asynchronous on `stream`."""
        _check(self._h, N.rt_lib().rt_scene_occluded_device(
            self._h, C.c_void_p(rays_ptr or None), int(n), float(t_min), float(t_max),
            C.c_void_p(t_max_each_ptr or None), C.c_void_p(out_ptr or None), C.c_void_p(stream or None)))

    def render_ao(self, camera: N.rt_camera, settings: RenderSettings, chain: int = 8,
                  radius: float = float("inf")) -> np.ndarray:
        """rt_render_ao -> [H][W] f64 sums of the 0/1 visibility over the settings' sample range, row 0 = bottom;
        `chain` as render_features'; `radius`: how far an occluder counts (> 0, inf accepted)."""
        out = np.zeros((camera.image_height, camera.image_width), dtype=np.float64)
        p = settings.params()
        _check(self._h, N.rt_lib().rt_render_ao(self._h, C.byref(camera), C.byref(p), int(chain), float(radius),
                                                out.ctypes.data))
        return out

    def render_ao_device(self, camera, settings: RenderSettings, chain: int, radius: float, ao_ptr: int,
                         stream: int = 0):
        """rt_render_ao_device: device [H][W] f64 output; asynchronous on `stream`."""
        p = settings.params()
        _check(self._h, N.rt_lib().rt_render_ao_device(self._h, C.byref(camera), C.byref(p), int(chain), float(radius),
                                                       C.c_void_p(ao_ptr or None), C.c_void_p(stream or None)))

    def lights(self):
        """rt_scene_lights of the uploaded scene -> (list of rt_light in object order, n_unlisted): the emitters
        render_direct samples, and how many emitters the listing rule leaves out (include/shirley_rt.h)."""
        n, u = C.c_int32(), C.c_int32()
        _check(self._h, N.rt_lib().rt_scene_lights(self._h, C.byref(n), C.byref(u), None))
        out = (N.rt_light * max(1, n.value))()
        _check(self._h, N.rt_lib().rt_scene_lights(self._h, C.byref(n), C.byref(u), out))
        return list(out[:n.value]), u.value

    def render_direct(self, camera: N.rt_camera, settings: RenderSettings, chain: int = 8):
        """rt_render_direct -> (emission, direct): [H][W][3] f64 sums over the settings' sample range, row 0 =
        bottom, of what the feature vertex emits and of the one-light-sample estimate of its direct
        illumination from the listed lights; `chain` as render_features'."""
        shape = (camera.image_height, camera.image_width, 3)
        em, di = np.zeros(shape, dtype=np.float64), np.zeros(shape, dtype=np.float64)
        p = settings.params()
        _check(self._h, N.rt_lib().rt_render_direct(self._h, C.byref(camera), C.byref(p), int(chain), em.ctypes.data,
                                                    di.ctypes.data))
        return em, di

    def render_direct_device(self, camera, settings: RenderSettings, chain: int, emission_ptr: int, direct_ptr: int,
                             stream: int = 0):
        """rt_render_direct_device: device [H][W][3] f64 outputs (0: not wanted; not both); asynchronous on
        `stream`."""
        p = settings.params()
        _check(self._h, N.rt_lib().rt_render_direct_device(
            self._h, C.byref(camera), C.byref(p), int(chain), C.c_void_p(emission_ptr or None),
            C.c_void_p(direct_ptr or None), C.c_void_p(stream or None)))

    def render_nee(self, camera: N.rt_camera, settings: RenderSettings, mis: bool = True) -> np.ndarray:
        """rt_render_nee -> [H][W][3] f64 sums over the settings' sample range, row 0 = bottom (render's layout):
        the path integrator with one light sample per Lambertian / FairyLight vertex; `mis` weights light sample
        and scatter by the balance heuristic (RT_NEE_MIS), else the light sample takes the listed lights whole."""
        out = np.zeros((camera.image_height, camera.image_width, 3), dtype=np.float64)
        p = settings.params()
        _check(self._h, N.rt_lib().rt_render_nee(self._h, C.byref(camera), C.byref(p), N.RT_NEE_MIS if mis else 0,
                                                 out.ctypes.data))
        return out

    def render_nee_device(self, camera, settings: RenderSettings, mis: bool, accum_ptr: int, stream: int = 0):
        """rt_render_nee_device: a device [H][W][3] f64 output; asynchronous on `stream`."""
        p = settings.params()
        _check(self._h, N.rt_lib().rt_render_nee_device(self._h, C.byref(camera), C.byref(p),
                                                        N.RT_NEE_MIS if mis else 0, C.c_void_p(accum_ptr or None),
                                                        C.c_void_p(stream or None)))

    def render_nee_adaptive(self, camera: N.rt_camera, settings: RenderSettings, adaptive: AdaptiveSettings,
                            mis: bool = True):
        """rt_render_nee_adaptive -> render_adaptive's tuple (accum, counts, moments, tile_error, report): one
        launch of the light-sampling integrator in which the wave that owns an 8x8 tile applies render_adaptive's
        stop rule; a pixel with n samples holds render_nee's samples [0, n), added batch by batch."""
        h, w = camera.image_height, camera.image_width
        accum = np.zeros((h, w, 3), dtype=np.float64)
        counts = np.zeros((h, w), dtype=np.int32)
        moments = np.zeros((h, w, 2), dtype=np.float64)
        tile_error = np.zeros(((h + 7) // 8, (w + 7) // 8), dtype=np.float64)
        report = N.rt_adaptive_report()
        p, a = settings.params(), adaptive.params()
        _check(self._h, N.rt_lib().rt_render_nee_adaptive(
            self._h, C.byref(camera), C.byref(p), N.RT_NEE_MIS if mis else 0, C.byref(a), accum.ctypes.data,
            counts.ctypes.data, moments.ctypes.data, tile_error.ctypes.data, C.byref(report)))
        return accum, counts, moments, tile_error, report

    def render_nee_adaptive_device(self, camera, settings: RenderSettings, adaptive: AdaptiveSettings, mis: bool,
                                   accum_ptr: int, counts_ptr: int, moments_ptr: int, tile_error_ptr: int = 0,
                                   stream: int = 0):
        """rt_render_nee_adaptive_device: device [H][W][3] f64, [H][W] int32, [H][W][2] f64 and (or 0) [tiles] f64
        outputs; asynchronous on `stream`."""
        p, a = settings.params(), adaptive.params()
        _check(self._h, N.rt_lib().rt_render_nee_adaptive_device(
            self._h, C.byref(camera), C.byref(p), N.RT_NEE_MIS if mis else 0, C.byref(a),
            C.c_void_p(accum_ptr or None), C.c_void_p(counts_ptr or None), C.c_void_p(moments_ptr or None),
            C.c_void_p(tile_error_ptr or None), C.c_void_p(stream or None)))

    def light_pick(self, cells: int) -> N.rt_light_grid:
        """rt_scene_light_pick: how render_direct / render_nee pick their one light per vertex until the next
        upload().  cells = 0: uniformly; 1 ... 64: from the light grid with that many cells along its longest
        axis (include/shirley_rt.h).  Returns the grid's dimensions and box."""
        info = N.rt_light_grid()
        _check(self._h, N.rt_lib().rt_scene_light_pick(self._h, int(cells), C.byref(info)))
        return info

    def light_pick_at(self, points: np.ndarray, xi: np.ndarray):
        """rt_light_pick_at: the device's pick alone -> (light [n] int32, prob [n] f64) for the vertices points[i]
        and the draws xi[i], in the grid last set by light_pick."""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        x = np.ascontiguousarray(xi, dtype=np.float64).reshape(-1)
        if len(p) != len(x):
            raise ValueError("one draw per point")
        light = np.zeros(max(1, len(p)), dtype=np.int32)
        prob = np.zeros(max(1, len(p)), dtype=np.float64)
        _check(self._h, N.rt_lib().rt_light_pick_at(self._h, len(p), p.ctypes.data, x.ctypes.data, light.ctypes.data,
                                                     prob.ctypes.data))
        return light[:len(p)], prob[:len(p)]

    def light_visibility(self, rays: int, seed: int) -> N.rt_light_visibility:
        """rt_scene_light_visibility: traces `rays` (1, 2, 4, 8, 16 or 32) shadow rays from every cell of the grid
        last set by light_pick to every listed light and weights the rows by what they saw, until the next
        upload(), light_pick() or light_visibility(); rays = 0 puts the plain rows back.  Returns the report."""
        rep = N.rt_light_visibility()
        _check(self._h, N.rt_lib().rt_scene_light_visibility(self._h, int(rays), int(seed), C.byref(rep)))
        self._light_vis_pairs = int(rep.pairs)  # (the size of light_visibility_masks' buffer)
        return rep

    def light_visibility_masks(self) -> np.ndarray:
        """rt_light_visibility_masks: the masks the device traced for the setting in force, flat [cells][n_lights]
        uint32 in the grid of the last light_pick (bit i: ray i of the pair)."""
        pairs = getattr(self, "_light_vis_pairs", 0)
        masks = np.zeros(max(1, pairs), dtype=np.uint32)
        _check(self._h, N.rt_lib().rt_light_visibility_masks(self._h, masks.ctypes.data))
        return masks[:pairs]

    def light_sampling(self, mode: int) -> None:
        """rt_scene_light_sampling: how render_direct / render_nee sample a light until the next upload():
        N.RT_LIGHT_SAMPLE_AREA (a point of its area), N.RT_LIGHT_SAMPLE_SOLID_ANGLE (a sphere light: a direction of
        the cone it subtends from the vertex; rects by area) or N.RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL (that, and a rect
        light: a direction of the spherical rectangle it subtends; include/shirley_rt.h)."""
        _check(self._h, N.rt_lib().rt_scene_light_sampling(self._h, int(mode)))

    def light_sample_at(self, points: np.ndarray, normals: np.ndarray, seed: int):
        """rt_light_sample_at: the device's light sample without its shadow ray -> rt_light_sample array, vertex i
        on the path key (seed, pixel = i, sample 0), under the pick and mode last set."""
        p, n = _vertices(points, normals)
        out = (N.rt_light_sample * max(1, len(p)))()
        _check(self._h, N.rt_lib().rt_light_sample_at(self._h, len(p), p.ctypes.data, n.ctypes.data, int(seed), out))
        return out[:len(p)]

    def probe(self, rays: np.ndarray, seed: int, sample: int = 0, draw: int = 0):
        """One iteration of ray_color's loop (render.rs:30-46) per ray through the megakernel's device code
        (rt_probe_segment): ray i on the path key (seed, pixel = i, sample, draw) -> rt_probe array
        (closest object, emitted / scatter of its material or the sky, the draw counter after it)."""
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        out = (N.rt_probe * max(1, len(r)))()
        _check(self._h, N.rt_lib().rt_probe_segment(self._h, r.ctypes.data, len(r), int(seed), int(sample),
                                                     int(draw), out))
        return out[:len(r)]

    def synchronize(self):
        _check(self._h, N.rt_lib().rt_synchronize(self._h))

    # ---- multi-GPU (rt_comm_*, rt_render_sharded) ----
    def comm_init_rank(self, unique_id: bytes, world: int, rank: int) -> "Comm":
        """This device as rank `rank` of a `world`-rank RCCL communicator (one process per GPU)."""
        if len(unique_id) != N.RT_COMM_ID_BYTES:
            raise ValueError("unique id must be RT_COMM_ID_BYTES bytes (rt_comm_unique_id)")
        buf = (C.c_uint8 * N.RT_COMM_ID_BYTES).from_buffer_copy(unique_id)
        h = C.c_void_p()
        _check(self._h, N.rt_lib().rt_comm_init_rank(self._h, buf, int(world), int(rank), C.byref(h)))
        return Comm(h, world, rank)

    def render_sharded(self, comm: "Comm", camera, settings: RenderSettings, accum_ptr: int = 0, stream: int = 0):
        """This rank's share of the frame + the RCCL gather; rank 0 receives the [H][W][3] sums at accum_ptr."""
        p = settings.params()
        _check(self._h, N.rt_lib().rt_render_sharded(self._h, comm.handle, C.byref(camera), C.byref(p),
                                                     C.c_void_p(accum_ptr or None), C.c_void_p(stream or None)))

    def counters(self) -> N.rt_counters:
        c = N.rt_counters()
        _check(self._h, N.rt_lib().rt_counters_get(self._h, C.byref(c)))
        return c


class Comm:
    """An rt_comm (one rank of an RCCL communicator)."""

    def __init__(self, handle, world: int, rank: int):
        self.handle, self.world, self.rank = handle, world, rank

    def close(self):
        if getattr(self, "handle", None):
            N.rt_lib().rt_comm_destroy(self.handle)
            self.handle = None

    __del__ = close


def comm_unique_id() -> bytes:
    """rt_comm_unique_id: the RCCL id rank 0 creates and hands to every rank."""
    buf = (C.c_uint8 * N.RT_COMM_ID_BYTES)()
    code = N.rt_lib().rt_comm_unique_id(buf)
    if code:
        raise N.RtError(code, "rt_comm_unique_id failed (RCCL unavailable or no device)")
    return bytes(buf)


def render_multi(devices, camera: N.rt_camera, settings: RenderSettings) -> np.ndarray:
    """rt_render_multi: the whole frame on several devices of this process (RCCL gather to devices[0])."""
    out = np.zeros((camera.image_height, camera.image_width, 3), dtype=np.float64)
    arr = (C.c_void_p * len(devices))(*[d.handle for d in devices])
    p = settings.params()
    _check(devices[0].handle, N.rt_lib().rt_render_multi(arr, len(devices), C.byref(camera), C.byref(p),
                                                         out.ctypes.data))
    return out


def scene_digest(scene: Scene, bvh: str = "reference") -> int:
    """rt_scene_digest_host: the digest rt_scene_upload would record for this scene (no device needed)."""
    builder = {"reference": N.RT_BVH_REFERENCE, "sah": N.RT_BVH_SAH}[bvh]
    d = C.c_uint64()
    code = N.rt_lib().rt_scene_digest_host(scene.desc_ptr, builder, C.byref(d))
    if code:
        raise N.RtError(code, "rt_scene_digest_host: invalid scene")
    return d.value


def light_grid_host(scene: Scene, cells: int):
    """rt_light_grid_host -> (rt_light_grid, cdf): the light grid rt_scene_light_pick would build for this scene
    (no device needed); cdf is [n[2]][n[1]][n[0]][n_lights] f64, empty when the scene lists no light."""
    info = N.rt_light_grid()
    code = N.rt_lib().rt_light_grid_host(scene.desc_ptr, int(cells), C.byref(info), None)
    if code:
        raise N.RtError(code, "rt_light_grid_host: invalid scene or cells, or a table of more than 2^22 entries")
    cdf = np.zeros((info.n[2], info.n[1], info.n[0], info.n_lights), dtype=np.float64)
    if cdf.size:
        code = N.rt_lib().rt_light_grid_host(scene.desc_ptr, int(cells), C.byref(info), cdf.ctypes.data)
        if code:
            raise N.RtError(code, "rt_light_grid_host failed")
    return info, cdf


def light_visibility_rays_host(scene: Scene, cells: int, rays: int, seed: int, cell: int, light: int):
    """rt_light_visibility_rays_host -> (rays [K][6] f64 = x, w; traced [K] uint8): the K rays of one (cell, light)
    pair of Device.light_visibility(rays, seed) after light_pick(cells), in plain C++ (no device needed)."""
    out = np.zeros((max(1, int(rays)), 6), dtype=np.float64)
    traced = np.zeros(max(1, int(rays)), dtype=np.uint8)
    code = N.rt_lib().rt_light_visibility_rays_host(scene.desc_ptr, int(cells), int(rays), int(seed), int(cell),
                                                    int(light), out.ctypes.data, traced.ctypes.data)
    if code:
        raise N.RtError(code, "rt_light_visibility_rays_host: invalid scene, cells, rays, cell or light")
    return out[:int(rays)], traced[:int(rays)]


def light_visibility_rows_host(scene: Scene, cells: int, rays: int, masks):
    """rt_light_visibility_rows_host -> cdf [n[2]][n[1]][n[0]][n_lights] f64: the rows Device.light_visibility
    builds from these masks ([cells][n_lights] uint32), in plain C++ (no device needed)."""
    info, _ = light_grid_host(scene, cells)
    m = np.ascontiguousarray(masks, dtype=np.uint32).reshape(-1)
    cdf = np.zeros((info.n[2], info.n[1], info.n[0], info.n_lights), dtype=np.float64)
    if m.size != cdf.size or not cdf.size:
        raise ValueError("one mask per (cell, light) of a scene that lists a light")
    code = N.rt_lib().rt_light_visibility_rows_host(scene.desc_ptr, int(cells), int(rays), m.ctypes.data,
                                                    cdf.ctypes.data)
    if code:
        raise N.RtError(code, "rt_light_visibility_rows_host: invalid scene, cells or rays")
    return cdf


def _vertices(points, normals):
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
    if len(p) != len(n):
        raise ValueError("one normal per point")
    return p, n


def light_sample_host(scene: Scene, cells: int, mode: int, points, normals, seed: int):
    """rt_light_sample_host -> rt_light_sample array: what Device.light_sample_at computes after light_pick(cells)
    and light_sampling(mode), in plain C++ (no device needed)."""
    p, n = _vertices(points, normals)
    out = (N.rt_light_sample * max(1, len(p)))()
    code = N.rt_lib().rt_light_sample_host(scene.desc_ptr, int(cells), int(mode), len(p), p.ctypes.data,
                                           n.ctypes.data, int(seed), out)
    if code:
        raise N.RtError(code, "rt_light_sample_host: invalid scene, cells or mode, or no listed light")
    return out[:len(p)]


def tile_layout(camera: N.rt_camera, world: int):
    n, m = C.c_int32(), C.c_int32()
    code = N.rt_lib().rt_tile_layout(C.byref(camera), int(world), C.byref(n), C.byref(m))
    if code:
        raise N.RtError(code, "rt_tile_layout failed")
    return n.value, m.value


def to_image(accum: np.ndarray, samples: int) -> np.ndarray:
    """image::to_image (image.rs:31-44): [H][W][3] sums -> RGB8 with row 0 = top."""
    h, w, _ = accum.shape
    a = np.ascontiguousarray(accum, dtype=np.float64)
    out = np.zeros((h, w, 3), dtype=np.uint8)
    code = N.rt_lib().rt_tonemap(a.ctypes.data, w, h, int(samples), out.ctypes.data)
    if code:
        raise N.RtError(code, "rt_tonemap failed")
    return out


def to_image_counts(accum: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """rt_tonemap_counts: to_image with each pixel's own sample count (an adaptive frame); count 0 -> black."""
    h, w, _ = accum.shape
    a = np.ascontiguousarray(accum, dtype=np.float64)
    n = np.ascontiguousarray(counts, dtype=np.int32).reshape(h, w)
    out = np.zeros((h, w, 3), dtype=np.uint8)
    code = N.rt_lib().rt_tonemap_counts(a.ctypes.data, n.ctypes.data, w, h, out.ctypes.data)
    if code:
        raise N.RtError(code, "rt_tonemap_counts failed")
    return out


def write_png(path: str, rgb8: np.ndarray):
    a = np.ascontiguousarray(rgb8, dtype=np.uint8)
    N.host_check(N.host_lib().sh_write_png(path.encode(), a.ctypes.data, a.shape[1], a.shape[0]))


def render_scene(settings: RenderSettings, scene: Scene, camera: N.rt_camera, output: Optional[str] = None,
                 device: Optional[Device] = None, bvh: str = "reference") -> np.ndarray:
    """render_scene (main.rs:65-130): samples 0 -> 1, render, to_image + PNG when ``output`` is set."""
    if settings.samples == 0:
        settings = RenderSettings(**{**settings.__dict__, "samples": 1})
    dev = device or Device(0)
    dev.upload(scene, bvh)
    accum = dev.render(camera, settings)
    if output:
        write_png(output, to_image(accum, settings.samples))
    return accum
