// rt_ctx.h — the context behind the C ABI's opaque rt_ctx / rt_comm, and the helpers that rt_api.cpp
// (scene, render, queries) and rt_multi.cpp (multi-GPU) share.  Internal to the library.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/shirley_rt.h"
#include "keycheck.h"
#include "light_pick.h"
#include "rccl_loader.h"
#include "rt_launch.h"
#include "rt_layout.h"
#include "scene_compile.h"

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// A rank of an RCCL communicator (multi-GPU frame sharding).
struct rt_comm {
  ncclComm_t comm = nullptr;
  int world = 1, rank = 0, device = 0;
  // rt_render_sharded's cross-rank check (keycheck.h): the key the ranks last agreed on, and the gathered
  // (digest, key) words of the last two calls in pinned host memory ([2 slots][world + 1][2]: the gathered
  // words, then this rank's own), each slot's copy marked by an event
  rt::KeyState ks;
  uint64_t* key_words = nullptr;
  hipEvent_t key_ev[2] = {nullptr, nullptr};
  int key_slot = 0;       // slot of the next call
  int key_pending = 0;    // slot of the pending (deferred) check
};

struct rt_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int cu_count = 0;
  // scene
  bool have_scene = false;
  rt::DScene scene{};
  DevBuf nodes, nodes4, prims, mats, texs, perlin, texels, exts;
  DevBuf ground;  // the ground-stack record and its guard bitmap (place.hop_kind == 2; rt_layout.h DGround)
  DevBuf planes;  // the plane record of a plane stack (place.hop_planes; rt_layout.h DPlanes)
  // the scene's light list (rt_scene_lights): the public records, and their device copies (DLight) that
  // rt_render_direct hands to its kernel as an argument of its own
  DevBuf lights;
  DevBuf prim_light;  // rt_render_nee: device primitive number -> light-list index or -1, its own argument too
  std::vector<rt_light> light_list;
  // rt_scene_light_pick: the host copies of the device records (the grid is built from them), the setting
  // (light_cells == 0: the uniform pick), the uploaded rows and the grid as the kernels take it
  std::vector<rt::DLight> light_dev;
  int32_t light_cells = 0;
  DevBuf light_cdf;
  rt::DLightGrid light_grid{};
  rt_light_grid light_grid_info{};
  int32_t light_sampling = RT_LIGHT_SAMPLE_AREA;  // rt_scene_light_sampling: how the passes sample a light
  // rt_scene_light_visibility: the report of the setting in force (rays == 0: off, the rows are the plain grid's),
  // the masks the device traced ([cells][L], kept for rt_light_visibility_masks) and the kernel's output buffer
  // (the masks, then the per-wave counts of traced rays)
  rt_light_visibility light_vis{};
  std::vector<uint32_t> light_vis_masks;
  DevBuf light_vis_out;
  int32_t n_unlisted_lights = 0;
  rt_scene_stats stats{};
  int blocks_per_cu = 0;
  rt::ScenePlacement place;        // the uploaded scene's plan (place.mk_threads: the megakernel block size)
  int split_nt = 0;                // RT_ENGINE_SPLIT: traversal waves per block (0: scene not eligible)
  int split_refill = 8;            // idle traversal lanes before a traversal wave claims rays
  // wavefront engine: the scene with its LDS node count sized for the extend block
  rt::DScene wf_scene{};
  int wf_blocks_per_cu = 0;
  bool wf_wide = false;      // wavefront extend runs the 4-wide scene-in-LDS kernel (wf_extend4)
  int wf4_blocks_per_cu = 0;
  bool has_perlin = false;
  int n_perlin = 0;
  // per-render scratch
  DevBuf partial, accum, counters, unit_counter, kcam;
  DevBuf moments, tile_list, tile_err;  // rt_render_adaptive: [H][W][2] moments, a step's tile list and its errors
  // rt_render_nee_adaptive: the tile counter's word, then (host form) the [H][W] counts; the moments of a host
  // call that asked for none
  DevBuf nee_adapt, nee_moments;
  DevBuf dn_a, dn_b;  // rt_denoise_device: the two [H][W][12] record buffers an iteration reads / writes
  DevBuf feat;        // rt_render_features: the device buffers behind the host copies
  DevBuf shutter0;  // {0, 0}: the shutter of rt_scene_hit / rt_probe_segment queries (DScene.shutter)
  DevBuf wf_pool, wf_iters;          // path slots (SoA) + texture queue; per-iteration counters ring
  uint32_t* wf_host = nullptr;       // pinned readback of the retired-slot count, one word per batch
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  hipEvent_t wf_ev[2] = {nullptr, nullptr};
  std::vector<hipEvent_t> lap_ev;    // RT_ENGINE_TIMING: one event after every launch
  bool have_timing = false;
  int last_engine = 0, last_iters = 0, last_timing = 0, last_chunk = 0, last_n_chunks = 0, last_passes = 0;
  uint64_t last_slots = 0, last_scratch = 0;
  std::vector<hipEvent_t> pass_ev;   // before / after the trace launch of each sample pass
  std::vector<rt::KBlock> host_blocks;    // host sources of the device KBlocks (KParams.kconst)
  uint64_t digest = 0;               // rt_scene_digest of the uploaded scene
  // device primitive number -> object index (primitives are numbered in the reference tree's leaf order)
  std::vector<int32_t> prim_object;
  // flattened rotated spheres (flat_object): object index -> RotateY's cos, sin, for rt_scene_hit's u, v
  std::vector<std::pair<int32_t, std::pair<double, double>>> uv_fixups;
  uint64_t host_samples = 0;  // samples of a frame served without a trace kernel (max_depth == 0)
  double lap_ms[3] = {0, 0, 0};
  // multi-GPU: this rank's packed tiles, the root's gathered buffer, and (root of rt_render_multi)
  // the communicators of the device set last used, kept for the next call
  DevBuf packed, gathered, parts, band, digests;
  std::vector<int> group_devices;
  std::vector<rt_comm> group_comms;
};

namespace rt {

inline int fail(rt_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

#define HIP_TRY(ctx, expr)                                                                      \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return fail(ctx, e_ == hipErrorOutOfMemory ? RT_E_OOM : RT_E_HIP, "%s: %s (%s:%d)", #expr, \
                  hipGetErrorString(e_), __FILE__, __LINE__);                                   \
  } while (0)

// rt_api.cpp
DCamera device_camera(const rt_camera* c);
int ensure(rt_ctx* c, DevBuf& b, size_t bytes);
void release(DevBuf& b);
int upload(rt_ctx* c, DevBuf& b, const void* src, size_t bytes);

inline int resolve_stream(rt_ctx* c, void* stream, hipStream_t* out) {
  *out = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  return RT_OK;
}

struct Layout {
  int tiles_x, tiles_y, n_tiles, n_tiles_rank;
};

inline Layout layout(const rt_camera* cam, int ty0, int ty1, int rank, int world) {
  Layout L;
  L.tiles_x = (cam->image_width + kTile - 1) / kTile;
  L.tiles_y = ty1 - ty0;
  L.n_tiles = L.tiles_x * L.tiles_y;
  L.n_tiles_rank = (L.n_tiles > rank) ? (L.n_tiles - rank + world - 1) / world : 0;
  return L;
}

// The sample range [begin, end) of a call (rt_render_params.sample_begin / sample_count, ABI 6).
struct SampleRange {
  int begin = 0, end = 0;
};

// An adaptive step (rt_render_adaptive) as render_window runs it: the megakernel renders the listed tiles
// (DWork.tile_list) and fold_stats_kernel takes the reduce's place — out_dev is the whole frame's [H][W][3]
// sums, continued in chunk order like a later sample pass; one chunk is one batch.
struct TileStep {
  const uint32_t* list_dev;  // ascending global tile indices (device)
  int n_list;
  double* moments_dev;       // [H][W][2]
  double* err_dev;           // [n_list]: the listed tiles' errors after the step
  long long batches_before;  // batches every listed pixel holds before the step
  int batch;                 // samples per batch (the step's unit length)
  double noise_floor;
};

// rt_api.cpp
int check_render_args(rt_ctx* c, const rt_camera* cam, const rt_render_params* p);
int resolve_range(rt_ctx* c, const rt_render_params* p, SampleRange* r);
int render_window(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const SampleRange& R, int ty0, int ty1,
                  int row0, int row1, int packed, double* out_dev, hipStream_t s, const TileStep* step = nullptr);

// The device forms of the tile passes (rt_render_{features,ao,direct,nee}_device) open with pass_check and, after
// their own argument checks, go on with pass_begin (pass_range, then pass_device), so every entry point keeps the
// order in which its refusals win; `name` is the entry point's, for the messages.
inline int check_single_rank(rt_ctx* c, const rt_render_params* p, const char* name) {
  return p->tile_world != 1 ? fail(c, RT_E_INVALID, "%s: tile_world must be 1", name) : RT_OK;
}
// The light grid the light-sampling passes hand to their kernel: null while the pick is uniform.
inline const DLightGrid* pass_light_grid(const rt_ctx* c) {
  return c->light_cells > 0 && !c->light_list.empty() ? &c->light_grid : nullptr;
}
// ... and their instances' sample kind (rt_scene_light_sampling: the mode's value is kSampleArea, kSampleCone or
// kSampleAll of light_cone.h / light_rect.h).
inline int pass_light_sample(const rt_ctx* c) { return c->light_sampling; }
inline int pass_check(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const char* name) {
  const int st = check_render_args(c, cam, p);
  return st ? st : check_single_rank(c, p, name);
}
inline int pass_range(rt_ctx* c, const rt_render_params* p, const char* name, SampleRange* R) {
  if (resolve_range(c, p, R)) return RT_E_INVALID;
  if (c->scene.exts) return fail(c, RT_E_UNSUPPORTED, "%s: scenes with book-2 objects are not supported", name);
  return RT_OK;
}
inline int pass_device(rt_ctx* c, void* stream, hipStream_t* s) {
  resolve_stream(c, stream, s);
  HIP_TRY(c, hipSetDevice(c->device));
  return RT_OK;
}
inline int pass_begin(rt_ctx* c, const rt_render_params* p, void* stream, const char* name, SampleRange* R,
                      hipStream_t* s) {
  const int st = pass_range(c, p, name, R);
  return st ? st : pass_device(c, stream, s);
}

// Their host-buffer forms: check_host_pass, the pass's own checks, then pass_to_host, which lays the planes out
// in c->feat (a plane without a host buffer keeps its place and gets a null device pointer), runs the device
// form on c->stream, copies the wanted planes back and synchronises.
inline int check_host_pass(rt_ctx* c, const rt_camera* cam) {
  if (!c) return RT_E_INVALID;
  if (!cam) return fail(c, RT_E_INVALID, "camera/params is NULL");
  if (cam->image_width < 1 || cam->image_height < 1) return fail(c, RT_E_INVALID, "bad image size");
  return RT_OK;
}
struct HostPlane {
  double* host;
  size_t count;  // doubles
  double* dev = nullptr;
};
template <class F>
int pass_to_host(rt_ctx* c, HostPlane* planes, int n, F device_form) {
  size_t total = 0;
  for (int i = 0; i < n; ++i) total += planes[i].count;
  int st = ensure(c, c->feat, total * sizeof(double));
  if (st) return st;
  double* at = static_cast<double*>(c->feat.p);
  for (int i = 0; i < n; ++i) {
    planes[i].dev = planes[i].host ? at : nullptr;
    at += planes[i].count;
  }
  st = device_form();
  if (st) return st;
  for (int i = 0; i < n; ++i)
    if (planes[i].host)
      HIP_TRY(c, hipMemcpyAsync(planes[i].host, planes[i].dev, planes[i].count * sizeof(double), hipMemcpyDeviceToHost,
                                c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

}  // namespace rt
