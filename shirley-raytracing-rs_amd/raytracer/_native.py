"""ctypes mirror of include/shirley_rt.h (render ABI) and include/shirley_host.h (C++ host layer).

The shared libraries are built in-tree by ``make -C shirley-raytracing-rs_amd`` (see
``__graft_entry__.build``).  There is no fallback: if a library is missing, loading raises.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# SHIRLEY_LIB_DIR selects an alternative in-tree build (A/B experiments); default: <pkg>/lib
LIB_DIR = os.environ.get("SHIRLEY_LIB_DIR") or os.path.join(_PKG_ROOT, "lib")
BIN_DIR = os.path.join(_PKG_ROOT, "bin")

RT_OK, RT_E_INVALID, RT_E_HIP, RT_E_OOM, RT_E_UNSUPPORTED, RT_E_RCCL = 0, 1, 2, 3, 4, 5
RT_COMM_ID_BYTES = 128
RT_GEOM_SPHERE, RT_GEOM_RECT_XY, RT_GEOM_RECT_YZ, RT_GEOM_RECT_XZ, RT_GEOM_RECT_BOX = range(5)
RT_GEOM_MOVING_SPHERE = 5  # book-2 extension
RT_MAT_METAL, RT_MAT_DIELECTRIC, RT_MAT_LAMBERTIAN, RT_MAT_DIFFUSE_LIGHT, RT_MAT_FAIRY_LIGHT = range(5)
RT_MAT_ISOTROPIC = 5  # book-2 extension
RT_TEX_SOLID, RT_TEX_CHECKER, RT_TEX_PERLIN, RT_TEX_IMAGE = range(4)
RT_SKY_ABOVE, RT_SKY_FLAT, RT_SKY_NONE = range(3)
RT_BVH_REFERENCE, RT_BVH_SAH = 0, 1
RT_BVH_NODES_GLOBAL, RT_BVH_NODES_HALF_LDS, RT_BVH_NODES_LDS = 0x100, 0x200, 0x400
RT_ENGINE_AUTO, RT_ENGINE_MEGAKERNEL, RT_ENGINE_WAVEFRONT, RT_ENGINE_SPLIT, RT_ENGINE_TIMING = 0, 1, 2, 3, 0x10
RT_TRAVERSAL_BINARY, RT_TRAVERSAL_RENDER = 0, 1
RT_PARTITION_AUTO, RT_PARTITION_TILES, RT_PARTITION_SAMPLES = 0, 1, 2
RT_NEE_MIS = 1  # rt_render_nee flags
RT_LIGHT_SAMPLE_AREA, RT_LIGHT_SAMPLE_SOLID_ANGLE = 0, 1  # rt_scene_light_sampling modes
RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL = 3  # ... spheres and rects by solid angle (2 is not a mode)

_d3 = C.c_double * 3
_d6 = C.c_double * 6


class rt_object(C.Structure):
    _fields_ = [("geometry", C.c_int32), ("material", C.c_int32), ("p", _d6),
                # book-2 extensions (absent from the reference)
                ("medium", C.c_int32), ("transform", C.c_int32), ("q", C.c_double * 5), ("density", C.c_double),
                ("rotate_y_deg", C.c_double), ("offset", _d3)]


class rt_material(C.Structure):
    _fields_ = [("kind", C.c_int32), ("texture", C.c_int32), ("albedo", _d3), ("param", C.c_double)]


class rt_texture(C.Structure):
    _fields_ = [("kind", C.c_int32), ("odd", C.c_int32), ("even", C.c_int32), ("table", C.c_int32),
                ("color", _d3), ("scale", C.c_double)]


class rt_perlin_table(C.Structure):
    _fields_ = [("ranfloat", (C.c_double * 3) * 256), ("perm_x", C.c_int32 * 256),
                ("perm_y", C.c_int32 * 256), ("perm_z", C.c_int32 * 256)]


class rt_image(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb", C.POINTER(C.c_uint8))]


class rt_scene_desc(C.Structure):
    _fields_ = [("sky", C.c_int32), ("sky_color", _d3),
                ("n_objects", C.c_int32), ("objects", C.POINTER(rt_object)),
                ("n_materials", C.c_int32), ("materials", C.POINTER(rt_material)),
                ("n_textures", C.c_int32), ("textures", C.POINTER(rt_texture)),
                ("n_perlin", C.c_int32), ("perlin", C.POINTER(rt_perlin_table)),
                ("n_images", C.c_int32), ("images", C.POINTER(rt_image))]


class rt_camera(C.Structure):
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("height", C.c_double),
                ("width", C.c_double), ("focal_length", C.c_double), ("has_lens", C.c_int32),
                ("lens_radius", C.c_double), ("origin", _d3), ("w", _d3), ("u", _d3), ("v", _d3),
                ("focus_length", C.c_double), ("time0", C.c_double), ("time1", C.c_double)]


class rt_render_params(C.Structure):
    _fields_ = [("samples", C.c_int32), ("max_depth", C.c_int32), ("seed", C.c_uint64),
                ("tile_rank", C.c_int32), ("tile_world", C.c_int32), ("sample_chunk", C.c_int32),
                ("engine", C.c_int32),
                # ABI 6
                ("sample_begin", C.c_int32), ("sample_count", C.c_int32), ("partition", C.c_int32),
                ("scratch_mb", C.c_int32)]


class rt_scene_stats(C.Structure):
    _fields_ = [("n_objects", C.c_int32), ("n_nodes", C.c_int32), ("n_leaves", C.c_int32),
                ("depth", C.c_int32), ("device_bytes", C.c_int64),
                # ABI 4
                ("n_nodes4", C.c_int32), ("wide_block", C.c_int32), ("origin_limit", C.c_double),
                # ABI 9
                ("hop_pass", C.c_int32),
                # the former tail padding (ABI 11, size unchanged)
                ("hop_kind", C.c_int32)]


class rt_counters(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("segments", C.c_uint64), ("node_visits", C.c_uint64),
                ("prim_tests", C.c_uint64), ("kernel_ms", C.c_double), ("reduce_ms", C.c_double),
                ("engine", C.c_int32), ("iterations", C.c_int32), ("slots", C.c_uint64),
                ("extend_ms", C.c_double), ("shade_ms", C.c_double), ("texture_ms", C.c_double),
                # ABI 4
                ("sample_chunk", C.c_int32), ("n_chunks", C.c_int32),
                # ABI 6
                ("passes", C.c_int32), ("trace_launches", C.c_int32), ("scratch_bytes", C.c_uint64)]


class rt_adaptive_params(C.Structure):  # ABI 8
    _fields_ = [("min_samples", C.c_int32), ("step", C.c_int32), ("threshold", C.c_double),
                ("noise_floor", C.c_double)]


class rt_adaptive_report(C.Structure):  # ABI 8
    _fields_ = [("steps", C.c_int32), ("tiles", C.c_int32), ("tiles_converged", C.c_int32), ("pad", C.c_int32),
                ("samples", C.c_uint64), ("segments", C.c_uint64), ("kernel_ms", C.c_double),
                ("fold_ms", C.c_double)]


class rt_denoise_inputs(C.Structure):  # ABI 10
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32), ("feature_samples", C.c_int32),
                ("accum", C.c_void_p), ("counts", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p),
                ("depth", C.c_void_p), ("variance", C.c_void_p)]


class rt_denoise_params(C.Structure):  # ABI 10
    _fields_ = [("iterations", C.c_int32), ("normal_power_log2", C.c_int32), ("sigma_z", C.c_double),
                ("sigma_a", C.c_double), ("sigma_c", C.c_double), ("albedo_floor", C.c_double)]


class rt_light(C.Structure):  # the scene's light list (added within ABI 11)
    _fields_ = [("object", C.c_int32), ("geometry", C.c_int32), ("emitter", C.c_int32), ("pad", C.c_int32),
                ("area", C.c_double), ("color", _d3)]


class rt_light_grid(C.Structure):  # the light grid of rt_scene_light_pick (added within ABI 11)
    _fields_ = [("n", C.c_int32 * 3), ("n_lights", C.c_int32), ("lo", _d3), ("hi", _d3)]


class rt_light_sample(C.Structure):  # a light sample before its shadow ray (added within ABI 11)
    _fields_ = [("light", C.c_int32), ("flags", C.c_int32), ("draws", C.c_uint32), ("pad", C.c_int32), ("w", _d3),
                ("cx", C.c_double), ("cy", C.c_double), ("g_plain", C.c_double), ("g_mis", C.c_double)]


class rt_light_visibility(C.Structure):  # the report of rt_scene_light_visibility (added within ABI 11)
    _fields_ = [("rays", C.c_int32), ("pad", C.c_int32), ("seed", C.c_uint64), ("pairs", C.c_uint64),
                ("traced", C.c_uint64), ("unoccluded", C.c_uint64), ("dead_points", C.c_uint64),
                ("kernel_ms", C.c_double)]


class rt_bvh_node(C.Structure):
    _fields_ = [("box", _d6), ("leaf", C.c_int32), ("lhs", C.c_int32), ("rhs", C.c_int32), ("pad", C.c_int32)]


class rt_hit(C.Structure):
    _fields_ = [("object", C.c_int32), ("front_face", C.c_int32), ("t", C.c_double), ("point", _d3),
                ("normal", _d3), ("u", C.c_double), ("v", C.c_double)]


class rt_probe(C.Structure):
    _fields_ = [("object", C.c_int32), ("front_face", C.c_int32), ("scattered", C.c_int32), ("emits", C.c_int32),
                ("draw", C.c_uint32), ("pad", C.c_int32), ("t", C.c_double), ("point", _d3), ("normal", _d3),
                ("emitted", _d3), ("attenuation", _d3), ("origin", _d3), ("direction", _d3)]


class sh_camera_spec(C.Structure):
    _fields_ = [("width", C.c_int32), ("ratio_num", C.c_int32), ("ratio_den", C.c_int32),
                ("vfov", C.c_double), ("focal_length", C.c_double), ("has_aperture", C.c_int32),
                ("aperture", C.c_double), ("look_from", _d3), ("look_at", _d3), ("up", _d3),
                ("override_focus", C.c_int32), ("focus_length", C.c_double),
                ("time0", C.c_double), ("time1", C.c_double)]


# every symbol declared in include/shirley_rt.h, with its C signature
RT_SIGNATURES = {
    "rt_version": (C.c_char_p, []),
    "rt_device_count": (C.c_int, [C.POINTER(C.c_int32)]),
    "rt_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "rt_destroy": (C.c_int, [C.c_void_p]),
    "rt_last_error": (C.c_char_p, [C.c_void_p]),
    "rt_scene_upload": (C.c_int, [C.c_void_p, C.POINTER(rt_scene_desc), C.c_int32]),
    "rt_scene_stats_get": (C.c_int, [C.c_void_p, C.POINTER(rt_scene_stats)]),
    "rt_scene_hop_instance": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "rt_scene_digest": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rt_scene_digest_host": (C.c_int, [C.POINTER(rt_scene_desc), C.c_int32, C.POINTER(C.c_uint64)]),
    "rt_render": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params), C.c_void_p]),
    "rt_render_scanlines": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params),
                                      C.c_int32, C.c_int32, C.c_void_p]),
    "rt_tile_layout": (C.c_int, [C.POINTER(rt_camera), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rt_render_device": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params), C.c_void_p,
                                   C.c_void_p]),
    "rt_render_tiles_device": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params),
                                         C.c_void_p, C.c_void_p]),
    "rt_unpack_tiles_device": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "rt_scene_hit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.POINTER(rt_hit)]),
    "rt_scene_hit_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                  C.POINTER(rt_hit)]),
    "rt_probe_segment": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32, C.c_uint32,
                                   C.POINTER(rt_probe)]),
    "rt_synchronize": (C.c_int, [C.c_void_p]),
    "rt_comm_unique_id": (C.c_int, [C.c_void_p]),
    "rt_comm_init_rank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "rt_comm_destroy": (C.c_int, [C.c_void_p]),
    "rt_render_sharded": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params),
                                    C.c_void_p, C.c_void_p]),
    "rt_render_multi": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(rt_camera), C.POINTER(rt_render_params),
                                  C.c_void_p]),
    "rt_counters_get": (C.c_int, [C.c_void_p, C.POINTER(rt_counters)]),
    "rt_bvh_build_host": (C.c_int, [C.POINTER(rt_scene_desc), C.c_int32, C.POINTER(C.c_int32),
                                    C.POINTER(rt_bvh_node), C.POINTER(C.c_int32)]),
    "rt_tonemap": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rt_tonemap_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_void_p]),
    "rt_render_adaptive": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params),
                                     C.POINTER(rt_adaptive_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(rt_adaptive_report)]),
    "rt_tonemap_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "rt_tonemap_counts_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_void_p]),
    # ABI 10
    "rt_render_features": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params), C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_features_device": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params), C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_denoise": (C.c_int, [C.POINTER(rt_denoise_inputs), C.POINTER(rt_denoise_params), C.c_void_p]),
    "rt_denoise_device": (C.c_int, [C.c_void_p, C.POINTER(rt_denoise_inputs), C.POINTER(rt_denoise_params),
                                    C.c_void_p, C.c_void_p]),
    "rt_moments_variance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rt_moments_variance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_void_p]),
    # ABI 11
    "rt_scene_occluded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p,
                                    C.c_void_p]),
    "rt_scene_occluded_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "rt_render_ao": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params), C.c_int32, C.c_double,
                               C.c_void_p]),
    "rt_render_ao_device": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params), C.c_int32,
                                      C.c_double, C.c_void_p, C.c_void_p]),
    # added within ABI 11: the light list and the direct-lighting pass
    "rt_scene_lights": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(rt_light)]),
    "rt_scene_lights_host": (C.c_int, [C.POINTER(rt_scene_desc), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(rt_light)]),
    "rt_render_direct": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params), C.c_int32,
                                   C.c_void_p, C.c_void_p]),
    "rt_render_direct_device": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params), C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    # added within ABI 11: the light-sampling path integrator
    "rt_render_nee": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params), C.c_int32,
                                C.c_void_p]),
    "rt_render_nee_device": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params), C.c_int32,
                                       C.c_void_p, C.c_void_p]),
    # added within ABI 11: the adaptive light-sampling render
    "rt_render_nee_adaptive": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params), C.c_int32,
                                         C.POINTER(rt_adaptive_params), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.POINTER(rt_adaptive_report)]),
    "rt_render_nee_adaptive_device": (C.c_int, [C.c_void_p, C.POINTER(rt_camera), C.POINTER(rt_render_params),
                                                C.c_int32, C.POINTER(rt_adaptive_params), C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    # added within ABI 11: the spatially weighted light pick
    "rt_light_grid_host": (C.c_int, [C.POINTER(rt_scene_desc), C.c_int32, C.POINTER(rt_light_grid), C.c_void_p]),
    "rt_scene_light_pick": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(rt_light_grid)]),
    "rt_light_pick_at": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # added within ABI 11: solid-angle sampling of sphere lights
    "rt_scene_light_sampling": (C.c_int, [C.c_void_p, C.c_int32]),
    "rt_light_sample_at": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64,
                                     C.POINTER(rt_light_sample)]),
    "rt_light_sample_host": (C.c_int, [C.POINTER(rt_scene_desc), C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_uint64, C.POINTER(rt_light_sample)]),
    # added within ABI 11: the visibility-aware light pick
    "rt_scene_light_visibility": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(rt_light_visibility)]),
    "rt_light_visibility_masks": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_light_visibility_rays_host": (C.c_int, [C.POINTER(rt_scene_desc), C.c_int32, C.c_int32, C.c_uint64, C.c_int32,
                                                C.c_int32, C.c_void_p, C.c_void_p]),
    "rt_light_visibility_rows_host": (C.c_int, [C.POINTER(rt_scene_desc), C.c_int32, C.c_int32, C.c_void_p,
                                                C.c_void_p]),
}

# every symbol declared in include/shirley_host.h
SH_SIGNATURES = {
    "sh_last_error": (C.c_char_p, []),
    "sh_scene_new": (C.c_void_p, []),
    "sh_scene_free": (None, [C.c_void_p]),
    "sh_scene_set_skybox": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]),
    "sh_scene_add_json": (C.c_int, [C.c_void_p, C.c_char_p]),
    "sh_scene_len": (C.c_int32, [C.c_void_p]),
    "sh_scene_to_json": (C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sh_scene_from_json": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "sh_scene_builtin": (C.c_int, [C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "sh_scene_finalize": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "sh_desc_view": (C.POINTER(rt_scene_desc), [C.c_void_p]),
    "sh_desc_free": (None, [C.c_void_p]),
    "sh_camera_build": (C.c_int, [C.POINTER(sh_camera_spec), C.POINTER(rt_camera)]),
    "sh_default_camera": (C.c_int, [C.c_int32, C.c_char_p, C.c_double, C.c_double, C.c_double,
                                    C.POINTER(rt_camera)]),
    "sh_cornell_camera": (C.c_int, [C.c_int32, C.POINTER(rt_camera)]),
    "sh_scene_camera": (C.c_int, [C.c_char_p, C.c_int32, C.c_char_p, C.c_double, C.c_double, C.c_double,
                                  C.POINTER(rt_camera)]),
    "sh_perlin_generate": (C.c_int, [C.c_uint64, C.c_uint32, C.POINTER(rt_perlin_table)]),
    "sh_write_png": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32]),
    "sh_load_image": (C.c_int, [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                C.POINTER(C.POINTER(C.c_uint8))]),
    "sh_free": (None, [C.c_void_p]),
}

_libs: dict = {}


def _load(name: str, sigs: dict):
    if name in _libs:
        return _libs[name]
    path = os.path.join(LIB_DIR, name)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `make -C {_PKG_ROOT}` "
                           "(or __graft_entry__.build()); there is no fallback path")
    lib = C.CDLL(path)
    for sym, (res, args) in sigs.items():
        fn = getattr(lib, sym)
        fn.restype = res
        fn.argtypes = args
    _libs[name] = lib
    return lib


def _single_hip_runtime():
    """PyTorch-ROCm bundles its own libamdhip64 (SONAME libamdhip64.so.7, but NEEDED as
    "libamdhip64.so"): if libshirley_rt.so pulled /opt/rocm's copy in first, a later torch import
    would load a second HIP/HSA runtime that finds no GPU.  Importing torch first makes our NEEDED
    libamdhip64.so.7 resolve to the runtime already in the process: one runtime, shared streams."""
    if os.environ.get("SHIRLEY_NO_TORCH") == "1":
        return
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def rt_lib():
    """libshirley_rt.so — the render boundary (HIP kernels)."""
    if "libshirley_rt.so" not in _libs:
        _single_hip_runtime()
    return _load("libshirley_rt.so", RT_SIGNATURES)


def host_lib():
    """libshirley_host.so — the C++ host layer (scenes, JSON, camera, PNG)."""
    return _load("libshirley_host.so", SH_SIGNATURES)


class RtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[rt status {code}] {msg}")
        self.code = code


def host_check(code: int):
    if code != 0:
        raise RtError(code, host_lib().sh_last_error().decode())
