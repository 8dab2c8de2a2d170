// rt_api.cpp — implementation of the C ABI in include/shirley_rt.h.
//
// Host side of the boundary: uploads the compiled scene (scene_compile.h: validation, BBox tree, HBM
// layout of rt_layout.h, placement plan), sizes the persistent launch and runs trace -> reduce on a HIP
// stream.  The multi-GPU entry points are in rt_multi.cpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "adaptive.h"
#include "plan.h"
#include "rt_ctx.h"

using namespace rt;

namespace rt {

int ensure(rt_ctx* c, DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return RT_OK;
  if (c) HIP_TRY(c, hipSetDevice(c->device));  // (rt_render_multi drives several devices from one thread)
  if (b.p) {
    (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
  }
  if (bytes == 0) return RT_OK;
  HIP_TRY(c, hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return RT_OK;
}

void release(DevBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.bytes = 0;
}

int upload(rt_ctx* c, DevBuf& b, const void* src, size_t bytes) {
  int st = ensure(c, b, std::max<size_t>(bytes, 16));
  if (st) return st;
  if (bytes) HIP_TRY(c, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return RT_OK;
}

DCamera device_camera(const rt_camera* c) {
  // camera/mod.rs:99-108, evaluated once with the reference's operation order (-ffp-contract=off)
  DCamera d{};
  d.width = c->image_width;
  d.height = c->image_height;
  d.has_lens = c->has_lens;
  d.lens_radius = c->lens_radius;
  d.wd = (double)c->image_width;
  d.hd = (double)c->image_height;
  d.inv_w = 1.0 / d.wd;  // correctly rounded (IEEE division)
  d.inv_h = 1.0 / d.hd;
  for (int k = 0; k < 3; ++k) {
    d.origin[k] = c->origin[k];
    d.u[k] = c->u[k];
    d.v[k] = c->v[k];
    d.horizontal[k] = c->u[k] * (c->width * c->focus_length);
    d.vertical[k] = c->v[k] * (c->height * c->focus_length);
  }
  for (int k = 0; k < 3; ++k)
    d.lower_left[k] = ((c->origin[k] - d.horizontal[k] * 0.5) - d.vertical[k] * 0.5) -
                      c->w[k] * (c->focal_length * c->focus_length);
  return d;
}

int check_render_args(rt_ctx* c, const rt_camera* cam, const rt_render_params* p) {
  if (!c) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "no scene uploaded (call rt_scene_upload first)");
  if (!cam || !p) return fail(c, RT_E_INVALID, "camera/params is NULL");
  if (cam->image_width < 1 || cam->image_height < 1 || cam->image_width > (1 << 16) || cam->image_height > (1 << 16))
    return fail(c, RT_E_INVALID, "bad image size %dx%d", cam->image_width, cam->image_height);
  if (p->samples < 0 || p->max_depth < 0) return fail(c, RT_E_INVALID, "negative samples/max_depth");
  if (p->tile_world < 1 || p->tile_rank < 0 || p->tile_rank >= p->tile_world)
    return fail(c, RT_E_INVALID, "bad tile rank/world %d/%d", p->tile_rank, p->tile_world);
  if (p->sample_chunk < 0) return fail(c, RT_E_INVALID, "negative sample_chunk");
  return RT_OK;
}

namespace {

constexpr long long kWfDefaultSlots = 1LL << 21;
constexpr int kWfBatch = 32;  // iterations launched between two host checks of the termination flag

int default_engine() {
  const char* e = getenv("SHIRLEY_ENGINE");
  if (e && !strcmp(e, "megakernel")) return RT_ENGINE_MEGAKERNEL;
  if (e && !strcmp(e, "wavefront")) return RT_ENGINE_WAVEFRONT;
  if (e && !strcmp(e, "split")) return RT_ENGINE_SPLIT;
  return RT_ENGINE_MEGAKERNEL;  // measured faster on MI355X
}

// Carve the slot arrays out of one allocation (each array 256-B aligned).
struct Carver {
  char* base;
  size_t off = 0;
  template <class T>
  T* take(size_t n) {
    off = (off + 255) & ~size_t(255);
    T* p = reinterpret_cast<T*>(base + off);
    off += n * sizeof(T);
    return p;
  }
};

size_t wf_pool_bytes(size_t n) {
  Carver cv{nullptr};
  for (int i = 0; i < 17; ++i) cv.take<double>(n);  // 15 path doubles + ht + tq.px/py/pz/scale below
  cv.take<uint64_t>(n);
  for (int i = 0; i < 11; ++i) cv.take<uint32_t>(n);
  cv.take<uint8_t>(n);
  for (int i = 0; i < 3; ++i) cv.take<double>(n);
  for (int i = 0; i < 3; ++i) cv.take<int32_t>(n);
  cv.take<unsigned long long>(2 * (n / kWave));  // unit windows
  cv.take<uint32_t>(n / kWave);                  // texture queue counts
  cv.take<unsigned>(64);                         // retired counter
  return cv.off + 256;
}

void wf_carve(void* base, size_t n, WfParams& P) {
  WfState& st = P.st;
  WfTexQ& tq = P.tq;
  Carver cv{static_cast<char*>(base)};
  double** dp[] = {&st.ox, &st.oy, &st.oz, &st.dx, &st.dy, &st.dz, &st.ax, &st.ay, &st.az,
                   &st.ex, &st.ey, &st.ez, &st.sx, &st.sy, &st.sz, &st.ht, &tq.px};
  for (double** q : dp) *q = cv.take<double>(n);
  st.part = cv.take<uint64_t>(n);
  st.pixel = cv.take<uint32_t>(n);
  st.sample = cv.take<uint32_t>(n);
  st.draw = cv.take<uint32_t>(n);
  st.c2 = cv.take<uint32_t>(n);
  st.c3 = cv.take<uint32_t>(n);
  st.s_next = cv.take<int32_t>(n);
  st.s_end = cv.take<int32_t>(n);
  st.depth = cv.take<int32_t>(n);
  st.hprim = cv.take<int32_t>(n);
  st.hface = cv.take<int32_t>(n);
  (void)cv.take<uint32_t>(n);  // spare
  st.state = cv.take<uint8_t>(n);
  tq.py = cv.take<double>(n);
  tq.pz = cv.take<double>(n);
  tq.scale = cv.take<double>(n);
  tq.slot = cv.take<int32_t>(n);
  tq.tex = cv.take<int32_t>(n);
  tq.kind = cv.take<int32_t>(n);
  P.win = cv.take<unsigned long long>(2 * (n / kWave));
  tq.count = cv.take<uint32_t>(n / kWave);
  P.retired = cv.take<unsigned>(64);
}

// The wavefront engine: start (every slot takes a unit and a camera ray), then rounds of
// extend -> shade -> texture until no slot holds work.  Rounds are launched in batches; the host
// reads the retired-slot count after the previous batch while the next batch runs, so the GPU
// never waits on the host.
int run_wavefront(rt_ctx* c, const KParams& kp, bool timing, hipStream_t s) {
  const uint64_t n_units = kp.work.n_units;
  long long slots = kWfDefaultSlots;
  if (const char* e = getenv("SHIRLEY_WF_SLOTS")) slots = std::max(64LL, atoll(e));
  slots = std::min<long long>(slots, std::max<long long>(64, (long long)n_units));
  slots = (slots + 63) / 64 * 64;
  const size_t n = (size_t)slots;
  int st = ensure(c, c->wf_pool, wf_pool_bytes(n));
  if (st) return st;
  st = ensure(c, c->wf_iters, sizeof(WfIter));  // extend cursors (wf_shade re-zeroes them each round)
  if (st) return st;

  WfParams P{};
  P.scene = c->wf_scene;
  P.scene.time0 = kp.scene.time0;
  P.scene.time1 = kp.scene.time1;
  P.scene.shutter = kp.scene.shutter;  // (the call's shutter, in the pass's KBlock)
  P.cam = kp.cam;
  P.work = kp.work;
  wf_carve(c->wf_pool.p, n, P);
  P.n_slots = (uint32_t)n;
  P.n_perlin = c->n_perlin;
  P.ext_window = 256;
  if (const char* e = getenv("SHIRLEY_WF_WINDOW")) P.ext_window = (uint32_t)std::max(1, atoi(e) / 64) * 64;
  P.partial = kp.partial;
  P.unit_counter = kp.unit_counter;
  P.counters = kp.counters;
  P.it = static_cast<WfIter*>(c->wf_iters.p);

  HIP_TRY(c, hipMemsetAsync(P.st.state, 0, n, s));           // kSlotIdle
  HIP_TRY(c, hipMemsetAsync(P.st.pixel, 0xff, n * 4, s));    // no unit
  HIP_TRY(c, hipMemsetAsync(P.it, 0, sizeof(WfIter), s));
  HIP_TRY(c, hipMemsetAsync(P.retired, 0, sizeof(unsigned), s));
  const int gt = wf_grid_threads();
  const int grid = (int)((n + gt - 1) / gt);
  const bool texture_pass = c->has_perlin;  // deferred entries exist only for Perlin leaves
  const int tex_grid = std::min(grid, 4 * c->cu_count);  // strided over slot groups, tables staged once per block
  const int ext_blocks = std::max(1, c->cu_count * std::max(1, c->wf_blocks_per_cu));

  // timing: an event before and after each launch of a round, elapsed times summed per kernel
  std::vector<hipEvent_t>& lap = c->lap_ev;
  std::vector<int> lap_tag;  // kernel the interval starting at this mark belongs to (3: none)
  auto lap_mark = [&](int tag) -> int {
    if (!timing) return RT_OK;
    if (lap_tag.size() == lap.size()) {
      hipEvent_t e;
      HIP_TRY(c, hipEventCreate(&e));
      lap.push_back(e);
    }
    HIP_TRY(c, hipEventRecord(lap[lap_tag.size()], s));
    lap_tag.push_back(tag);
    return RT_OK;
  };

  HIP_TRY(c, wf_start(P, grid, s));
  long long iter = 1;
  // safety bound: every round advances each working slot by one segment or one regeneration
  const long long max_iters = 64 + 2LL * ((long long)((n_units + n - 1) / n) + 1) *
                                       (long long)(kp.work.chunk) * (long long)(kp.work.max_depth + 2);
  int batch = 0;
  for (;;) {
    for (int k = 0; k < kWfBatch; ++k, ++iter) {
      if ((st = lap_mark(0))) return st;
      if (c->wf_wide)
        HIP_TRY(c, wf_launch_extend4(P, c->cu_count * c->wf4_blocks_per_cu, s));
      else
        HIP_TRY(c, wf_launch_extend(P, ext_blocks, s));
      if ((st = lap_mark(1))) return st;
      HIP_TRY(c, wf_launch_shade(P, grid, s));
      if ((st = lap_mark(2))) return st;
      if (texture_pass) HIP_TRY(c, wf_launch_texture(P, tex_grid, s));
      if ((st = lap_mark(3))) return st;
    }
    HIP_TRY(c, hipMemcpyAsync(&c->wf_host[batch & 1], P.retired, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipEventRecord(c->wf_ev[batch & 1], s));
    if (batch > 0) {
      HIP_TRY(c, hipEventSynchronize(c->wf_ev[(batch - 1) & 1]));
      if (c->wf_host[(batch - 1) & 1] >= (uint32_t)n) break;  // every slot retired
    }
    ++batch;
    if (iter > max_iters) return fail(c, RT_E_HIP, "wavefront engine did not terminate after %lld rounds", iter);
  }
  c->last_iters += (int)iter;
  c->last_slots = n;
  c->last_timing = timing;
  if (timing && !lap_tag.empty()) {
    HIP_TRY(c, hipEventSynchronize(lap[lap_tag.size() - 1]));
    double acc[3] = {0, 0, 0};
    for (size_t i = 0; i + 1 < lap_tag.size(); ++i) {
      if (lap_tag[i] > 2) continue;
      float ms = 0.f;
      HIP_TRY(c, hipEventElapsedTime(&ms, lap[i], lap[i + 1]));
      acc[lap_tag[i]] += ms;
    }
    for (int k = 0; k < 3; ++k) c->lap_ms[k] += acc[k];  // (summed over the call's sample passes)
  }
  return RT_OK;
}

}  // namespace

int resolve_range(rt_ctx* c, const rt_render_params* p, SampleRange* r) {
  const int S = p->samples == 0 ? 1 : p->samples;  // main.rs:75-80
  if (p->sample_begin < 0 || p->sample_count < 0 || p->sample_begin > S ||
      (long long)p->sample_begin + p->sample_count > S)
    return fail(c, RT_E_INVALID, "sample range [%d, +%d) outside [0, %d)", p->sample_begin, p->sample_count, S);
  r->begin = p->sample_begin;
  r->end = p->sample_count ? p->sample_begin + p->sample_count : S;
  return RT_OK;
}

// trace + reduce of samples [R.begin, R.end) for tile rows [ty0, ty1); out layout: packed tiles
// (packed=1) or rows [row0, row1).  The call's work units (pixel x chunk of samples) are traced in
// sample passes of at most `scratch` bytes of partial sums each; every pass's reduce continues the
// per-pixel chunk-order sums of the passes before it (reduce_kernel `accumulate`), so the frame is the
// same for any number of passes.  `step` (an adaptive step, rt_ctx.h): the listed tiles of the whole frame
// on the megakernel, folded into out_dev and the moments by fold_stats_kernel.
int render_window(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const SampleRange& R, int ty0, int ty1,
                  int row0, int row1, int packed, double* out_dev, hipStream_t s, const TileStep* step) {
  int st = check_render_args(c, cam, p);
  if (st) return st;
  HIP_TRY(c, hipSetDevice(c->device));
  const int count = R.end - R.begin;
  Layout L = layout(cam, ty0, ty1, p->tile_rank, p->tile_world);
  if (step) {
    if (ty0 != 0 || packed || p->tile_world != 1 || step->n_list < 1 || step->n_list > L.n_tiles)
      return fail(c, RT_E_INVALID, "bad adaptive step");
    L.n_tiles_rank = step->n_list;
  }
  const long long n_pix = (long long)L.n_tiles_rank * kTilePixels;

  int engine = p->engine & 0xf;
  const bool timing = (p->engine & RT_ENGINE_TIMING) != 0;
  if (engine == RT_ENGINE_AUTO) engine = default_engine();
  if (engine != RT_ENGINE_MEGAKERNEL && engine != RT_ENGINE_WAVEFRONT && engine != RT_ENGINE_SPLIT)
    return fail(c, RT_E_INVALID, "bad engine %d", p->engine);
  if (engine == RT_ENGINE_SPLIT && c->split_nt == 0) engine = RT_ENGINE_MEGAKERNEL;  // scene not eligible
  if (step && engine != RT_ENGINE_MEGAKERNEL)
    return fail(c, RT_E_UNSUPPORTED, "tile lists are rendered by the megakernel only (engine %d)", engine);

  const long long lanes = (long long)c->cu_count * std::max(1, c->blocks_per_cu) * c->place.mk_threads;
  long long budget = (long long)(p->scratch_mb > 0 ? p->scratch_mb : kDefaultScratchMiB) << 20;
  if (p->scratch_mb == 0)
    if (const char* e = getenv("SHIRLEY_SCRATCH_MB")) budget = std::max(1LL, atoll(e)) << 20;  // tuning
  SamplePlan plan = plan_samples(n_pix, count, engine, lanes, p->sample_chunk, budget);
  if (const char* e = getenv("SHIRLEY_SEGMENTS"))  // (tuning: per-block unit segments forced on / off)
    plan.segments = engine == RT_ENGINE_MEGAKERNEL && atoi(e) != 0;
  if (!plan.ok) return fail(c, RT_E_UNSUPPORTED, "frame too large (%lld pixels)", (long long)n_pix);
  // a device short of memory gets more, smaller passes instead of a failed call (the frame is the same
  // for any number of passes)
  // (SHIRLEY_SIMULATE_OOM_MB, tests only: a partial buffer above that many MiB fails like hipMalloc would)
  long long oom_limit = 0;
  if (const char* e = getenv("SHIRLEY_SIMULATE_OOM_MB")) oom_limit = atoll(e) << 20;
  auto alloc_partial = [&](size_t bytes) {
    if (oom_limit > 0 && (long long)bytes > oom_limit)
      return fail(c, RT_E_OOM, "simulated out-of-memory: %zu bytes of partial sums", bytes);
    return ensure(c, c->partial, bytes);
  };
  bool fell_back = false;
  const std::string err_before = c->err;
  while ((st = alloc_partial((size_t)plan.partial_bytes)) == RT_E_OOM && plan.per_pass > 1) {
    (void)hipGetLastError();
    fell_back = true;
    plan = plan_samples(n_pix, count, engine, lanes, p->sample_chunk, plan.partial_bytes / 2);
  }
  if (st) return st;
  if (fell_back) c->err = err_before;  // the call succeeds: the refused allocation leaves no message behind
  const int chunk = plan.chunk, n_chunks = plan.n_chunks, passes = plan.passes, per_pass = plan.per_pass;
  const size_t partial_bytes = (size_t)plan.partial_bytes;

  KParams kp{};
  kp.scene = c->scene;
  kp.scene.time0 = cam->time0;  // book-2 shutter (ray time side stream)
  kp.scene.time1 = cam->time1;
  kp.cam = device_camera(cam);
  kp.work.tiles_x = L.tiles_x;
  kp.work.tiles_y = L.tiles_y;
  kp.work.ty0 = ty0;
  kp.work.tile_rank = p->tile_rank;
  kp.work.tile_world = p->tile_world;
  kp.work.n_tiles_rank = L.n_tiles_rank;
  kp.work.chunk = chunk;
  kp.work.max_depth = p->max_depth;
  kp.work.seed = p->seed;
  kp.work.div_tiles_x = make_udiv((uint32_t)L.tiles_x);
  kp.work.tile_list = step ? step->list_dev : nullptr;
  kp.partial = static_cast<double*>(c->partial.p);
  kp.counters = static_cast<DCounters*>(c->counters.p);

  // the megakernel's per-pass KBlock (KParams.kconst): device copies of the camera, the scene record, the
  // pass's work descriptor and the output / queue / statistics pointers; their host sources stay alive in
  // the ctx until the next call
  st = ensure(c, c->kcam, (size_t)passes * sizeof(KBlock));
  if (st) return st;
  // every kernel of the call reads the shutter from pass 0's device copy of the scene record
  kp.scene.shutter = &static_cast<KBlock*>(c->kcam.p)->scene.time0;
  c->host_blocks.assign(passes, KBlock{});
  const uint64_t nseg = (uint64_t)std::max(1, c->cu_count * std::max(1, c->blocks_per_cu));
  {
    const size_t bytes = std::max<size_t>(64, (size_t)nseg * sizeof(uint32_t));
    st = ensure(c, c->unit_counter, bytes);
    if (st) return st;
    kp.unit_counter = static_cast<unsigned long long*>(c->unit_counter.p);
  }
  if ((int)c->pass_ev.size() < 2 * passes) {
    const size_t have = c->pass_ev.size();
    c->pass_ev.resize(2 * passes, nullptr);
    for (size_t i = have; i < c->pass_ev.size(); ++i) HIP_TRY(c, hipEventCreate(&c->pass_ev[i]));
  }
  HIP_TRY(c, hipMemsetAsync(c->counters.p, 0, kCounterSlots * sizeof(DCounters), s));
  c->last_engine = engine;
  c->host_samples = 0;
  c->last_chunk = chunk;
  c->last_n_chunks = n_chunks;
  c->last_passes = 0;
  c->last_scratch = partial_bytes;
  c->last_iters = 0;
  c->last_slots = 0;
  c->last_timing = 0;
  for (double& x : c->lap_ms) x = 0.0;
  HIP_TRY(c, hipEventRecord(c->ev[0], s));
  const bool trace = n_pix > 0 && count > 0 && p->max_depth > 0;
  if (step && (!trace || chunk != step->batch)) return fail(c, RT_E_INVALID, "bad adaptive step");
  if (!trace) {
    // nothing to trace: ray_color's loop never runs with max_depth == 0 (render.rs:30: every sample is
    // black), or the range is empty.  The window is written by a reduce over no chunks (zeros); the
    // samples counter counts the window's in-image pixels of this rank's tiles, as the kernel would.
    uint64_t inside = 0;
    for (long long lt = 0; lt < L.n_tiles_rank; ++lt) {
      const long long gt = lt * p->tile_world + p->tile_rank;
      const int tx = (int)(gt % L.tiles_x), ty = ty0 + (int)(gt / L.tiles_x);
      const int w = std::min(kTile, cam->image_width - tx * kTile), h = std::min(kTile, cam->image_height - ty * kTile);
      if (w > 0 && h > 0) inside += (uint64_t)w * (uint64_t)h;
    }
    c->host_samples = inside * (uint64_t)count;
    HIP_TRY(c, hipEventRecord(c->ev[1], s));
    if (n_pix > 0)
      HIP_TRY(c, launch_reduce(kp.partial, 0, L.n_tiles_rank, L.tiles_x, ty0, p->tile_rank, p->tile_world,
                               cam->image_width, row0, row1, packed, 0, out_dev, s));
    HIP_TRY(c, hipEventRecord(c->ev[2], s));
    c->have_timing = true;
    return RT_OK;
  }
  for (int k = 0; k < passes; ++k) {
    const int c0 = k * per_pass, c1 = std::min(n_chunks, c0 + per_pass);
    DWork& w = kp.work;
    w.sample_base = R.begin + c0 * chunk;
    w.samples = (int)std::min<long long>(R.end, (long long)R.begin + (long long)c1 * chunk);
    w.n_chunks = c1 - c0;
    w.n_units = (uint64_t)n_pix * (uint64_t)w.n_chunks;
    w.div_unit_tile = make_udiv((uint32_t)w.n_chunks * (uint32_t)kTilePixels);
    // per-block unit segments (trace.hip; plan.h): one counter per megakernel block
    const uint64_t per = (w.n_units + nseg - 1) / nseg;
    w.n_segs = plan.segments ? (uint32_t)nseg : 0u;
    w.seg_len = (uint32_t)std::max<uint64_t>(kSegmentWindow, (per + kSegmentWindow - 1) / kSegmentWindow * kSegmentWindow);
    w.q_window = plan.queue_window;
    if (const char* e = getenv("SHIRLEY_WINDOW"))  // (tuning: the shared queue's window, units)
      w.q_window = (uint32_t)std::max(1, atoi(e) / kWave) * (uint32_t)kWave;
    // the device copy is taken after every field is set (the kernel may read any of them)
    KBlock& kb = c->host_blocks[k];
    kb.cam = kp.cam;
    kb.scene = kp.scene;
    kb.work = w;
    kb.partial = kp.partial;
    kb.unit_counter = kp.unit_counter;
    kb.counters = kp.counters;
    kb.ground = c->place.hop_kind == 2 ? static_cast<const DGround*>(c->ground.p) : nullptr;
    kb.planes = c->place.hop_planes ? static_cast<const DPlanes*>(c->planes.p) : nullptr;
    void* kdev = static_cast<KBlock*>(c->kcam.p) + k;
    HIP_TRY(c, hipMemcpyAsync(kdev, &kb, sizeof(KBlock), hipMemcpyHostToDevice, s));
    kp.kconst = (uint64_t)(uintptr_t)kdev;
    HIP_TRY(c, hipMemsetAsync(c->unit_counter.p, 0, std::max<size_t>(64, (size_t)nseg * sizeof(uint32_t)), s));
    HIP_TRY(c, hipEventRecord(c->pass_ev[2 * k], s));
    if (engine == RT_ENGINE_WAVEFRONT) {
      st = run_wavefront(c, kp, timing, s);
      if (st) return st;
    } else if (engine == RT_ENGINE_SPLIT) {
      kp.split_refill = c->split_refill;
      KParams ks = kp;  // (the split engine's LDS layout holds no material tables)
      ks.scene.n_lds_mats = ks.scene.n_lds_texs = 0;
      HIP_TRY(c, launch_split(ks, c->split_nt, c->cu_count, s));
    } else {
      HIP_TRY(c, launch_trace(kp, (int)nseg, c->place.mk_threads, hop_instance(c->place), s));
    }
    HIP_TRY(c, hipEventRecord(c->pass_ev[2 * k + 1], s));
    if (k == passes - 1) HIP_TRY(c, hipEventRecord(c->ev[1], s));
    if (step)
      HIP_TRY(c, launch_fold_stats(kp.partial, w.n_chunks, step->n_list, step->list_dev, L.tiles_x, cam->image_width,
                                   cam->image_height, step->batches_before + c1, step->batch, step->noise_floor,
                                   out_dev, step->moments_dev, step->err_dev, s));
    else
      HIP_TRY(c, launch_reduce(kp.partial, w.n_chunks, L.n_tiles_rank, L.tiles_x, ty0, p->tile_rank, p->tile_world,
                               cam->image_width, row0, row1, packed, k > 0 ? 1 : 0, out_dev, s));
    c->last_passes = k + 1;
  }
  HIP_TRY(c, hipEventRecord(c->ev[2], s));
  c->have_timing = true;
  return RT_OK;
}

}  // namespace rt

extern "C" {

const char* rt_version(void) { return "shirley-rt 0.2 (gfx950, f64 wavefront + persistent megakernel)"; }

int rt_device_count(int32_t* out) {
  if (!out) return RT_E_INVALID;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  *out = (e == hipSuccess) ? n : 0;
  return e == hipSuccess ? RT_OK : RT_E_HIP;
}

const char* rt_last_error(const rt_ctx* ctx) { return ctx ? ctx->err.c_str() : "NULL context"; }

int rt_create(int32_t device, rt_ctx** out) {
  if (!out) return RT_E_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return RT_E_HIP;
  if (device < 0 || device >= n) return RT_E_INVALID;
  rt_ctx* c = new rt_ctx();
  c->device = device;
  auto bail = [&](int code) {
    rt_destroy(c);
    return code;
  };
  if (hipSetDevice(device) != hipSuccess) return bail(RT_E_HIP);
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail(RT_E_HIP);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return bail(RT_E_HIP);
  c->cu_count = prop.multiProcessorCount;
  for (auto& e : c->ev)
    if (hipEventCreate(&e) != hipSuccess) return bail(RT_E_HIP);
  for (auto& e : c->wf_ev)
    if (hipEventCreate(&e) != hipSuccess) return bail(RT_E_HIP);
  if (hipHostMalloc((void**)&c->wf_host, 64, hipHostMallocDefault) != hipSuccess) return bail(RT_E_OOM);
  if (ensure(c, c->counters, kCounterSlots * sizeof(DCounters)) || ensure(c, c->unit_counter, 64)) return bail(RT_E_OOM);
  *out = c;
  return RT_OK;
}

int rt_destroy(rt_ctx* c) {
  if (!c) return RT_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (DevBuf* b : {&c->nodes, &c->nodes4, &c->prims, &c->mats, &c->texs, &c->perlin, &c->texels, &c->exts, &c->ground, &c->planes, &c->lights, &c->prim_light, &c->light_cdf, &c->light_vis_out, &c->partial, &c->kcam, &c->shutter0, &c->moments, &c->tile_list, &c->tile_err, &c->nee_adapt, &c->nee_moments, &c->dn_a, &c->dn_b, &c->feat,
                    &c->accum, &c->counters, &c->unit_counter, &c->wf_pool, &c->wf_iters, &c->packed, &c->gathered,
                    &c->parts, &c->band, &c->digests})
    release(*b);
  for (rt_comm& m : c->group_comms)
    if (m.comm) (void)rccl().CommDestroy(m.comm);
  for (auto& e : c->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : c->wf_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : c->lap_ev) (void)hipEventDestroy(e);
  if (c->wf_host) (void)hipHostFree(c->wf_host);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return RT_OK;
}

int rt_scene_upload(rt_ctx* c, const rt_scene_desc* d, int32_t builder) {
  if (!c) return RT_E_INVALID;
  CompiledScene cs;
  int st = compile_scene(d, builder, tuning_from_env(), &cs, &c->err);
  if (st) return st;
  const ScenePlacement& P = cs.place;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->have_scene = false;
  auto up = [&](DevBuf& b, const auto& v) { return upload(c, b, v.data(), v.size() * sizeof v[0]); };
  if ((st = up(c->nodes, cs.nodes)) || (st = up(c->nodes4, cs.nodes4)) || (st = up(c->prims, cs.prims)) ||
      (st = up(c->mats, cs.mats)) || (st = up(c->texels, cs.texels)))
    return st;
  for (DTex& t : cs.texs)  // an image texture points at its image in the pool, now on the device
    if (t.kind == RT_TEX_IMAGE) t.img.texels = static_cast<const uint8_t*>(c->texels.p) + cs.img_off[t.table];
  if ((st = up(c->texs, cs.texs)) || (st = up(c->perlin, cs.perlin))) return st;
  if (!cs.exts.empty()) {
    if ((st = up(c->exts, cs.exts))) return st;
  } else {
    release(c->exts);
  }
  if (!cs.ground.empty()) {
    if ((st = up(c->ground, cs.ground))) return st;
  } else {
    release(c->ground);
  }
  if (!cs.planes.empty()) {
    if ((st = up(c->planes, cs.planes))) return st;
  } else {
    release(c->planes);
  }
  if (!cs.lights.dev.empty()) {
    if ((st = up(c->lights, cs.lights.dev))) return st;
  } else {
    release(c->lights);
  }
  if ((st = up(c->prim_light, cs.prim_light))) return st;
  if ((st = ensure(c, c->shutter0, 2 * sizeof(double)))) return st;
  HIP_TRY(c, hipMemset(c->shutter0.p, 0, 2 * sizeof(double)));

  DScene& S = c->scene;
  S.nodes = static_cast<const DNode*>(c->nodes.p);
  S.nodes4 = c->nodes4.p;
  S.prims = static_cast<const DPrim*>(c->prims.p);
  S.mats = static_cast<const DMat*>(c->mats.p);
  S.texs = static_cast<const DTex*>(c->texs.p);
  S.perlin = static_cast<const DPerlin*>(c->perlin.p);
  S.exts = cs.exts.empty() ? nullptr : static_cast<const DExt*>(c->exts.p);
  S.time0 = S.time1 = 0.0;  // the shutter comes with each render call's camera
  S.shutter = static_cast<const double*>(c->shutter0.p);
  S.n_nodes = (int32_t)cs.nodes.size();
  S.n_nodes4 = cs.stats.n_nodes4;
  S.n_prims = cs.stats.n_objects;
  place_scene(P, S);
  S.sky = d->sky;
  for (int k = 0; k < 3; ++k) S.sky_color[k] = d->sky_color[k];
  c->place = P;

  int bpc = 0;
  HIP_TRY(c, trace_occupancy(S, P.mk_threads, hop_instance(P), &bpc));
  if (bpc < 1) return fail(c, RT_E_UNSUPPORTED, "trace kernel does not fit on a CU (LDS %lld B)", P.stack_bytes);
  c->blocks_per_cu = bpc;
  // wavefront extend block: its own LDS node count, no material tables
  DScene W = S;
  W.n_lds_mats = W.n_lds_texs = 0;
  W.n_lds_nodes = P.wf_n_lds_nodes;
  int wbpc = 0;
  HIP_TRY(c, wf_prepare(W, &wbpc));
  if (wbpc < 1) return fail(c, RT_E_UNSUPPORTED, "wavefront extend kernel does not fit on a CU");
  c->wf_scene = W;
  c->wf_blocks_per_cu = wbpc;
  c->wf_wide = false;
  if (P.wf_extend4) {
    int b4 = 0;
    HIP_TRY(c, wf_prepare4(S, &b4));
    if (b4 >= 1) {
      c->wf_wide = true;
      c->wf4_blocks_per_cu = b4;
      c->wf_scene = S;  // wf_extend4 reads the megakernel's LDS layout (without the material tables)
      c->wf_scene.n_lds_mats = c->wf_scene.n_lds_texs = 0;
    }
  }
  c->split_nt = 0;
  if (P.split_nt) {
    if (P.split_refill) c->split_refill = P.split_refill;
    int sb = 0;
    if (split_supported_nt(P.split_nt)) HIP_TRY(c, split_prepare(S, P.split_nt, &sb));
    if (sb >= 1) c->split_nt = P.split_nt;
  }

  c->n_perlin = cs.n_perlin;
  c->has_perlin = cs.has_perlin;
  c->prim_object = std::move(cs.prim_object);
  c->uv_fixups = std::move(cs.uv_fixups);
  c->light_list = std::move(cs.lights.lights);
  c->light_dev = std::move(cs.lights.dev);
  c->light_cells = 0;  // every upload starts with the uniform pick (rt_scene_light_pick)
  c->light_sampling = RT_LIGHT_SAMPLE_AREA;  // ... and with area sampling (rt_scene_light_sampling)
  c->light_vis = rt_light_visibility{};       // ... and without visibility weights (rt_scene_light_visibility)
  c->light_vis_masks.clear();
  c->n_unlisted_lights = cs.lights.n_unlisted;
  c->stats = cs.stats;
  c->digest = cs.digest;
  c->have_scene = true;
  return RT_OK;
}
int rt_scene_digest(rt_ctx* c, uint64_t* out) {
  if (!c || !out) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "no scene uploaded");
  *out = c->digest;
  return RT_OK;
}

int rt_scene_digest_host(const rt_scene_desc* d, int32_t builder, uint64_t* out) {
  if (!d || !out) return RT_E_INVALID;
  if (validate(d, nullptr)) return RT_E_INVALID;
  *out = scene_digest(d, builder & ~kPlacementMask);
  return RT_OK;
}

int rt_scene_stats_get(rt_ctx* c, rt_scene_stats* out) {
  if (!c || !out) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "no scene uploaded");
  *out = c->stats;
  return RT_OK;
}

int rt_scene_hop_instance(rt_ctx* c, int32_t* out) {
  if (!c || !out) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "no scene uploaded");
  *out = hop_instance(c->place);
  return RT_OK;
}

int rt_tile_layout(const rt_camera* cam, int32_t world, int32_t* n_tiles_total, int32_t* max_tiles_per_rank) {
  if (!cam || world < 1 || cam->image_width < 1 || cam->image_height < 1) return RT_E_INVALID;
  int tiles_y = (cam->image_height + kTile - 1) / kTile;
  Layout L = layout(cam, 0, tiles_y, 0, world);
  if (n_tiles_total) *n_tiles_total = L.n_tiles;
  if (max_tiles_per_rank) *max_tiles_per_rank = (L.n_tiles + world - 1) / world;
  return RT_OK;
}

int rt_render_device(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, double* accum_dev, void* stream) {
  if (!accum_dev) return fail(c, RT_E_INVALID, "accum_dev is NULL");
  hipStream_t s;
  resolve_stream(c, stream, &s);
  int tiles_y = cam ? (cam->image_height + kTile - 1) / kTile : 0;
  SampleRange R;
  if (p && resolve_range(c, p, &R)) return RT_E_INVALID;
  return render_window(c, cam, p, R, 0, tiles_y, 0, cam ? cam->image_height : 0, 0, accum_dev, s);
}

int rt_render_tiles_device(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, double* packed_dev,
                           void* stream) {
  if (!packed_dev) return fail(c, RT_E_INVALID, "packed_dev is NULL");
  hipStream_t s;
  resolve_stream(c, stream, &s);
  int tiles_y = cam ? (cam->image_height + kTile - 1) / kTile : 0;
  SampleRange R;
  if (p && resolve_range(c, p, &R)) return RT_E_INVALID;
  return render_window(c, cam, p, R, 0, tiles_y, 0, cam ? cam->image_height : 0, 1, packed_dev, s);
}

int rt_unpack_tiles_device(rt_ctx* c, const rt_camera* cam, int32_t world, const double* gathered_dev,
                           double* accum_dev, void* stream) {
  if (!c || !cam || !gathered_dev || !accum_dev || world < 1) return fail(c, RT_E_INVALID, "bad unpack args");
  hipStream_t s;
  resolve_stream(c, stream, &s);
  int32_t n_total = 0, max_tiles = 0;
  rt_tile_layout(cam, world, &n_total, &max_tiles);
  int tiles_x = (cam->image_width + kTile - 1) / kTile;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, launch_unpack(gathered_dev, world, max_tiles, n_total, tiles_x, cam->image_width, cam->image_height,
                           accum_dev, s));
  return RT_OK;
}

int rt_render(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, double* accum_host) {
  if (!c) return RT_E_INVALID;
  if (!accum_host || !cam) return fail(c, RT_E_INVALID, "NULL argument");
  return rt_render_scanlines(c, cam, p, 0, cam->image_height, accum_host);
}

int rt_render_scanlines(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t line_begin,
                        int32_t line_end, double* rows_host) {
  if (!c) return RT_E_INVALID;
  if (!cam || !rows_host) return fail(c, RT_E_INVALID, "NULL argument");
  if (line_begin < 0 || line_end > cam->image_height || line_begin > line_end)
    return fail(c, RT_E_INVALID, "bad line range [%d, %d)", line_begin, line_end);
  if (line_begin == line_end) return RT_OK;
  if (p && p->tile_world != 1) return fail(c, RT_E_INVALID, "host-buffer render needs tile_world == 1");
  size_t bytes = (size_t)(line_end - line_begin) * cam->image_width * 3 * sizeof(double);
  int st = ensure(c, c->accum, bytes);
  if (st) return st;
  int ty0 = line_begin / kTile, ty1 = (line_end + kTile - 1) / kTile;
  SampleRange R;
  if (p && resolve_range(c, p, &R)) return RT_E_INVALID;
  st = render_window(c, cam, p, R, ty0, ty1, line_begin, line_end, 0, static_cast<double*>(c->accum.p), c->stream);
  if (st) return st;
  HIP_TRY(c, hipMemcpyAsync(rows_host, c->accum.p, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

int rt_scene_hit(rt_ctx* c, const double* rays, int32_t n, double t_min, double t_max, rt_hit* out) {
  return rt_scene_hit_ex(c, rays, n, t_min, t_max, RT_TRAVERSAL_BINARY, out);
}

int rt_scene_hit_ex(rt_ctx* c, const double* rays, int32_t n, double t_min, double t_max, int32_t traversal,
                    rt_hit* out) {
  if (!c) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "no scene uploaded");
  if (n < 0 || (n > 0 && (!rays || !out))) return fail(c, RT_E_INVALID, "bad ray batch");
  if (traversal != RT_TRAVERSAL_BINARY && traversal != RT_TRAVERSAL_RENDER)
    return fail(c, RT_E_INVALID, "bad traversal %d", traversal);
  if (n == 0) return RT_OK;
  static_assert(sizeof(rt_hit) == 80, "rt_hit layout");
  HIP_TRY(c, hipSetDevice(c->device));
  DevBuf r, h;
  int st = upload(c, r, rays, (size_t)n * 6 * sizeof(double));
  if (!st) st = ensure(c, h, (size_t)n * sizeof(rt_hit));
  if (!st) {
    const double* rd = static_cast<const double*>(r.p);
    hipError_t e = traversal == RT_TRAVERSAL_RENDER
                       ? launch_hit4(c->scene, c->place.wide, rd, n, t_min, t_max, h.p, c->stream)
                       : launch_hit(c->scene, rd, n, t_min, t_max, h.p, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, h.p, (size_t)n * sizeof(rt_hit), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) st = fail(c, RT_E_HIP, "rt_scene_hit: %s", hipGetErrorString(e));
  }
  if (!st)
    for (int32_t i = 0; i < n; ++i)
      if (out[i].object >= 0) out[i].object = c->prim_object[out[i].object];
  if (!st && !c->uv_fixups.empty())  // (sorted by object index)
    for (int32_t i = 0; i < n; ++i) {
      auto it = std::lower_bound(c->uv_fixups.begin(), c->uv_fixups.end(), out[i].object,
                                 [](const auto& f, int32_t o) { return f.first < o; });
      if (it != c->uv_fixups.end() && it->first == out[i].object) instance_sphere_uv(it->second.first, it->second.second, out[i]);
    }
  release(r);
  release(h);
  return st;
}

int rt_probe_segment(rt_ctx* c, const double* rays, int32_t n, uint64_t seed, uint32_t sample, uint32_t draw,
                     rt_probe* out) {
  if (!c) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "no scene uploaded");
  if (n < 0 || (n > 0 && (!rays || !out))) return fail(c, RT_E_INVALID, "bad ray batch");
  if (n == 0) return RT_OK;
  static_assert(sizeof(rt_probe) == 176, "rt_probe layout (trace.hip ProbeOut)");
  HIP_TRY(c, hipSetDevice(c->device));
  DevBuf r, h;
  int st = upload(c, r, rays, (size_t)n * 6 * sizeof(double));
  if (!st) st = ensure(c, h, (size_t)n * sizeof(rt_probe));
  if (!st) {
    DScene S = c->scene;
    S.time0 = S.time1 = 0.0;  // (book-2 ray time 0, like the oracle's or_probe_segment)
    hipError_t e = launch_probe(S, c->place.wide, static_cast<const double*>(r.p), n, seed,
                                sample, draw, h.p, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, h.p, (size_t)n * sizeof(rt_probe), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) st = fail(c, RT_E_HIP, "rt_probe_segment: %s", hipGetErrorString(e));
  }
  if (!st)
    for (int32_t i = 0; i < n; ++i)
      if (out[i].object >= 0) out[i].object = c->prim_object[out[i].object];
  release(r);
  release(h);
  return st;
}

int rt_synchronize(rt_ctx* c) {
  if (!c) return RT_E_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  return RT_OK;
}

int rt_counters_get(rt_ctx* c, rt_counters* out) {
  if (!c || !out) return RT_E_INVALID;
  std::memset(out, 0, sizeof *out);
  if (!c->have_timing) return fail(c, RT_E_INVALID, "no render has run on this context");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipEventSynchronize(c->ev[2]));
  std::vector<DCounters> dc(kCounterSlots);
  HIP_TRY(c, hipMemcpy(dc.data(), c->counters.p, kCounterSlots * sizeof(DCounters), hipMemcpyDeviceToHost));
  out->samples = c->host_samples;
  for (const DCounters& k : dc) {
    out->samples += k.samples;
    out->segments += k.segments;
    out->node_visits += k.node_visits;
    out->prim_tests += k.prim_tests;
  }
#ifdef RT_PHASE_TIMING
  {
    double ph[kPhBuckets] = {};
    for (const DCounters& k : dc)
      for (int i = 0; i < kPhBuckets; ++i) ph[i] += (double)k.pad[i];
    const int order[] = {kPhTrav, kPhDown, kPhRecord, kPhRegen, kPhMarble, kPhDraws, kPhCamera, kPhShade, kPhTail, kPhHop};
    const char* names[] = {"trav", "down", "record", "regen", "marble", "draws", "camera", "shade", "tail", "hop"};
    double tot = 0;
    for (int b : order) tot += ph[b];
    fprintf(stderr, "[phase] wave-time fractions:");
    for (int i = 0; i < 10; ++i) fprintf(stderr, " %s %.4f", names[i], ph[order[i]] / tot);
    fprintf(stderr, " (wave-cycles %.4g)\n", tot);
    const double lane = ph[kPhLaneSteps], wave = ph[kPhWaveSteps];
    fprintf(stderr, "[phase] traversal lane steps %.4g, wave steps %.4g, SIMD utilisation %.3f\n", lane, wave,
            lane / (64.0 * wave));
    phase_counters_dump();
  }
#endif
#ifdef RT_TIMELINE
  timeline_dump();
#endif
  // kernel_ms: the trace launches of the call (one per sample pass); reduce_ms: the rest of the call's
  // device time (the reduces)
  float all = 0.f;
  HIP_TRY(c, hipEventElapsedTime(&all, c->ev[0], c->ev[2]));
  double trace = 0.0;
  for (int k = 0; k < c->last_passes; ++k) {
    float t = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&t, c->pass_ev[2 * k], c->pass_ev[2 * k + 1]));
    trace += t;
  }
  out->kernel_ms = trace;
  out->reduce_ms = std::max(0.0, (double)all - trace);
  out->passes = c->last_passes;
  out->trace_launches = c->last_passes;
  out->scratch_bytes = c->last_scratch;
  out->engine = c->last_engine;
  out->sample_chunk = c->last_chunk;
  out->n_chunks = c->last_n_chunks;
  out->iterations = c->last_iters;
  out->slots = c->last_slots;
  if (c->last_timing) {
    out->extend_ms = c->lap_ms[0];
    out->shade_ms = c->lap_ms[1];
    out->texture_ms = c->lap_ms[2];
  }
  return RT_OK;
}

int rt_bvh_build_host(const rt_scene_desc* d, int32_t builder, int32_t* n_nodes, rt_bvh_node* nodes, int32_t* root) {
  if (!d || !n_nodes) return RT_E_INVALID;
  if (validate(d, nullptr)) return RT_E_INVALID;
  std::vector<rt_object> flat;
  const rt_scene_desc fd = flat_scene(d, flat);
  BuiltTree t = build_tree(&fd, builder, tuning_from_env());
  if (nodes) {
    if (*n_nodes < (int32_t)t.nodes.size()) return RT_E_INVALID;
    for (size_t i = 0; i < t.nodes.size(); ++i) {
      box_to6(t.nodes[i].box, nodes[i].box);
      nodes[i].leaf = t.nodes[i].leaf;
      nodes[i].lhs = t.nodes[i].lhs;
      nodes[i].rhs = t.nodes[i].rhs;
      nodes[i].pad = 0;
    }
  }
  *n_nodes = (int32_t)t.nodes.size();
  if (root) *root = t.root;
  return RT_OK;
}

int rt_tonemap(const double* accum, int32_t width, int32_t height, int32_t samples, uint8_t* rgb8) {
  if (!accum || !rgb8 || width < 1 || height < 1) return RT_E_INVALID;
  const double inv = 1.0 / (double)(samples == 0 ? 1 : samples);
  for (int32_t j = 0; j < height; ++j)
    for (int32_t i = 0; i < width; ++i) {
      const double* c = accum + ((size_t)j * width + i) * 3;
      uint8_t* o = rgb8 + ((size_t)(height - j - 1) * width + i) * 3;
      for (int k = 0; k < 3; ++k) {
        double y = std::sqrt(c[k] * inv) * 255.999;  // (x * COLOR_SCALE) as u8, color.rs:31-38
        o[k] = (std::isnan(y) || y <= 0.0) ? 0 : (y >= 255.0 ? 255 : (uint8_t)y);
      }
    }
  return RT_OK;
}

int rt_tonemap_device(rt_ctx* c, const double* accum_dev, int32_t width, int32_t height, int32_t samples,
                      uint8_t* rgb8_dev, void* stream) {
  if (!c || !accum_dev || !rgb8_dev || width < 1 || height < 1) return RT_E_INVALID;
  hipStream_t s;
  resolve_stream(c, stream, &s);
  HIP_TRY(c, hipSetDevice(c->device));
  const double inv = 1.0 / (double)(samples == 0 ? 1 : samples);
  HIP_TRY(c, launch_tonemap(accum_dev, width, height, inv, rgb8_dev, s));
  return RT_OK;
}

int rt_tonemap_counts(const double* accum, const int32_t* counts, int32_t width, int32_t height, uint8_t* rgb8) {
  if (!accum || !counts || !rgb8 || width < 1 || height < 1) return RT_E_INVALID;
  for (int32_t j = 0; j < height; ++j)
    for (int32_t i = 0; i < width; ++i) {
      const double* c = accum + ((size_t)j * width + i) * 3;
      uint8_t* o = rgb8 + ((size_t)(height - j - 1) * width + i) * 3;
      const int32_t n = counts[(size_t)j * width + i];
      const double inv = n > 0 ? 1.0 / (double)n : 0.0;
      for (int k = 0; k < 3; ++k) {
        double y = std::sqrt(c[k] * inv) * 255.999;  // rt_tonemap's arithmetic on the pixel's own count
        o[k] = (n <= 0 || std::isnan(y) || y <= 0.0) ? 0 : (y >= 255.0 ? 255 : (uint8_t)y);
      }
    }
  return RT_OK;
}

int rt_tonemap_counts_device(rt_ctx* c, const double* accum_dev, const int32_t* counts_dev, int32_t width,
                             int32_t height, uint8_t* rgb8_dev, void* stream) {
  if (!c || !accum_dev || !counts_dev || !rgb8_dev || width < 1 || height < 1) return RT_E_INVALID;
  hipStream_t s;
  resolve_stream(c, stream, &s);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, launch_tonemap_counts(accum_dev, counts_dev, width, height, rgb8_dev, s));
  return RT_OK;
}

// The step loop of an adaptive frame (adaptive.h) on the host, like the traversal stacks' sizing: after
// each step the listed tiles' errors come back, the tiles that go on make the next (sorted) list — one
// small round trip per step, a deterministic list and no device compaction.
int rt_render_adaptive(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_adaptive_params* a,
                       double* accum_host, int32_t* counts_host, double* moments_host, double* tile_error_host,
                       rt_adaptive_report* report) {
  if (!c) return RT_E_INVALID;
  if (!cam || !p || !a || !accum_host || !counts_host) return fail(c, RT_E_INVALID, "NULL argument");
  int st = check_render_args(c, cam, p);
  if (st) return st;
  AdaptivePlan plan;
  if (const char* why = adaptive_validate(p, a, &plan)) return fail(c, RT_E_INVALID, "rt_render_adaptive: %s", why);
  const int engine = p->engine & 0xf;
  if (engine == RT_ENGINE_WAVEFRONT || engine == RT_ENGINE_SPLIT)
    return fail(c, RT_E_UNSUPPORTED, "rt_render_adaptive: tile lists are rendered by the megakernel only (engine %d)", engine);
  if (engine != RT_ENGINE_AUTO && engine != RT_ENGINE_MEGAKERNEL) return fail(c, RT_E_INVALID, "bad engine %d", p->engine);

  const int W = cam->image_width, H = cam->image_height;
  const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile, n_tiles = tiles_x * tiles_y;
  const size_t n_px = (size_t)W * H;
  rt_adaptive_report rep{};
  rep.tiles = n_tiles;
  std::vector<int32_t> tile_count(n_tiles, 0);
  std::vector<double> tile_err(n_tiles, std::numeric_limits<double>::quiet_NaN());
  auto finish = [&]() {
    for (int j = 0; j < H; ++j)
      for (int i = 0; i < W; ++i) counts_host[(size_t)j * W + i] = tile_count[(j / kTile) * tiles_x + i / kTile];
    for (int t = 0; t < n_tiles; ++t) rep.tiles_converged += tile_continues(tile_err[t], plan.threshold) ? 0 : 1;
    if (tile_error_host) std::copy(tile_err.begin(), tile_err.end(), tile_error_host);
    if (report) *report = rep;
    return RT_OK;
  };
  if (p->max_depth == 0) {
    // ray_color's loop never runs (render.rs:30): every sample is black and there is nothing to estimate,
    // so every tile stops after the first step (whatever the threshold)
    std::fill(accum_host, accum_host + n_px * 3, 0.0);
    if (moments_host) std::fill(moments_host, moments_host + n_px * 2, 0.0);
    std::fill(tile_count.begin(), tile_count.end(), plan.min_samples);
    std::fill(tile_err.begin(), tile_err.end(), 0.0);
    rep.steps = 1;
    rep.samples = (uint64_t)n_px * (uint64_t)plan.min_samples;
    finish();
    if (report) report->tiles_converged = n_tiles;
    return RT_OK;
  }

  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if ((st = ensure(c, c->accum, n_px * 3 * sizeof(double))) || (st = ensure(c, c->moments, n_px * 2 * sizeof(double))) ||
      (st = ensure(c, c->tile_list, (size_t)n_tiles * sizeof(uint32_t))) ||
      (st = ensure(c, c->tile_err, (size_t)n_tiles * sizeof(double))))
    return st;
  HIP_TRY(c, hipMemsetAsync(c->accum.p, 0, n_px * 3 * sizeof(double), s));
  HIP_TRY(c, hipMemsetAsync(c->moments.p, 0, n_px * 2 * sizeof(double), s));

  rt_render_params q = *p;
  q.sample_chunk = plan.batch;
  q.engine = RT_ENGINE_MEGAKERNEL | (p->engine & RT_ENGINE_TIMING);
  std::vector<uint32_t> list(n_tiles);
  for (int t = 0; t < n_tiles; ++t) list[t] = (uint32_t)t;
  std::vector<double> err(n_tiles);
  const int n_steps = adaptive_n_steps(plan);
  for (int k = 0; k < n_steps && !list.empty(); ++k) {
    SampleRange R;
    adaptive_step_range(plan, k, &R.begin, &R.end);
    if (R.end <= R.begin) break;
    const size_t n_list = list.size();
    HIP_TRY(c, hipMemcpyAsync(c->tile_list.p, list.data(), n_list * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    TileStep ts{};
    ts.list_dev = static_cast<const uint32_t*>(c->tile_list.p);
    ts.n_list = (int)n_list;
    ts.moments_dev = static_cast<double*>(c->moments.p);
    ts.err_dev = static_cast<double*>(c->tile_err.p);
    ts.batches_before = R.begin / plan.batch;
    ts.batch = plan.batch;
    ts.noise_floor = plan.noise_floor;
    st = render_window(c, cam, &q, R, 0, tiles_y, 0, H, 0, static_cast<double*>(c->accum.p), s, &ts);
    if (st) return st;
    HIP_TRY(c, hipMemcpyAsync(err.data(), c->tile_err.p, n_list * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    rt_counters cnt;
    if ((st = rt_counters_get(c, &cnt))) return st;
    rep.steps += 1;
    rep.samples += cnt.samples;
    rep.segments += cnt.segments;
    rep.kernel_ms += cnt.kernel_ms;
    rep.fold_ms += cnt.reduce_ms;
    for (size_t i = 0; i < n_list; ++i) {
      tile_err[list[i]] = err[i];
      tile_count[list[i]] = R.end;
    }
    list.resize(adaptive_compact(list.data(), err.data(), n_list, plan.threshold, list.data()));
  }
  HIP_TRY(c, hipMemcpyAsync(accum_host, c->accum.p, n_px * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (moments_host)
    HIP_TRY(c, hipMemcpyAsync(moments_host, c->moments.p, n_px * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return finish();
}

}  // extern "C"
