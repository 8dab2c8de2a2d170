// rt_nee.cpp — the light-sampling path integrator of include/shirley_rt.h and its adaptive form (added within
// ABI 11; nee.hip, nee_adaptive.hip, nee_kernel.h, direct.h).
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "adaptive.h"
#include "rt_ctx.h"

using namespace rt;

extern "C" {

int rt_render_nee_device(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t flags, double* accum_dev,
                         void* stream) {
  int st = check_render_args(c, cam, p);
  if (st) return st;
  if (flags & ~(int32_t)RT_NEE_MIS) return fail(c, RT_E_INVALID, "rt_render_nee: unknown flag bits 0x%x", flags);
  if ((st = check_single_rank(c, p, "rt_render_nee"))) return st;  // (the flags are refused first: no pass_check)
  if (!accum_dev) return fail(c, RT_E_INVALID, "rt_render_nee: the output buffer is NULL");
  SampleRange R;
  hipStream_t s;
  if ((st = pass_begin(c, p, stream, "rt_render_nee", &R, &s))) return st;
  if (p->max_depth <= 0 || R.end <= R.begin) {  // no segment: zero sums
    const size_t n = (size_t)cam->image_width * cam->image_height * 3;
    HIP_TRY(c, hipMemsetAsync(accum_dev, 0, n * sizeof(double), s));
    return RT_OK;
  }
  const int n_lights = (int)c->light_list.size();
  HIP_TRY(c, launch_nee(c->scene, c->place.wide, (flags & RT_NEE_MIS) != 0, device_camera(cam), p->seed, R.begin, R.end,
                        p->max_depth, n_lights ? static_cast<const DLight*>(c->lights.p) : nullptr, n_lights,
                        pass_light_grid(c), pass_light_sample(c), static_cast<const int32_t*>(c->prim_light.p), accum_dev,
                        s));
  return RT_OK;
}

int rt_render_nee(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t flags, double* accum_host) {
  const int st = check_host_pass(c, cam);
  if (st) return st;
  if (!accum_host) return fail(c, RT_E_INVALID, "rt_render_nee: the output buffer is NULL");
  HostPlane pl{accum_host, (size_t)cam->image_width * cam->image_height * 3};
  return pass_to_host(c, &pl, 1, [&] { return rt_render_nee_device(c, cam, p, flags, pl.dev, c->stream); });
}

// ---- rt_render_nee_adaptive (nee_adaptive.hip) ----

// SHIRLEY_NEE_BLOCKS=N (tests and measurement; read per call): the adaptive launch's grid is N blocks in place of
// the device's fill (fewer or more), and never more than the tiles need
static int nee_blocks_cap() {
  const char* e = getenv("SHIRLEY_NEE_BLOCKS");
  return e ? std::max(0, atoi(e)) : 0;
}

int rt_render_nee_adaptive_device(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t flags,
                                  const rt_adaptive_params* a, double* accum_dev, int32_t* counts_dev,
                                  double* moments_dev, double* tile_error_dev, void* stream) {
  int st = check_render_args(c, cam, p);
  if (st) return st;
  if (flags & ~(int32_t)RT_NEE_MIS)
    return fail(c, RT_E_INVALID, "rt_render_nee_adaptive: unknown flag bits 0x%x", flags);
  AdaptivePlan plan;
  if (const char* why = adaptive_validate(p, a, &plan)) return fail(c, RT_E_INVALID, "rt_render_nee_adaptive: %s", why);
  if (!accum_dev || !counts_dev || !moments_dev)
    return fail(c, RT_E_INVALID, "rt_render_nee_adaptive: an output buffer is NULL");
  SampleRange R;
  hipStream_t s;
  if ((st = pass_begin(c, p, stream, "rt_render_nee_adaptive", &R, &s))) return st;
  const size_t n_px = (size_t)cam->image_width * cam->image_height;
  const int n_tiles = layout(cam, 0, (cam->image_height + kTile - 1) / kTile, 0, 1).n_tiles;
  if (p->max_depth <= 0) {  // no segment: zero sums and moments, every tile stops at min_samples with e = 0
    HIP_TRY(c, hipMemsetAsync(accum_dev, 0, n_px * 3 * sizeof(double), s));
    HIP_TRY(c, hipMemsetAsync(moments_dev, 0, n_px * 2 * sizeof(double), s));
    HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(counts_dev), plan.min_samples, n_px, s));
    if (tile_error_dev) HIP_TRY(c, hipMemsetAsync(tile_error_dev, 0, (size_t)n_tiles * sizeof(double), s));
    return RT_OK;
  }
  if ((st = ensure(c, c->nee_adapt, 64))) return st;
  HIP_TRY(c, hipMemsetAsync(c->nee_adapt.p, 0, sizeof(uint32_t), s));
  const NeeAdapt ad{static_cast<unsigned*>(c->nee_adapt.p), moments_dev, tile_error_dev, counts_dev, plan.batch,
                    plan.min_samples, plan.step, plan.threshold, plan.noise_floor};
  const int n_lights = (int)c->light_list.size();
  HIP_TRY(c, launch_nee_adaptive(c->scene, c->place.wide, (flags & RT_NEE_MIS) != 0, device_camera(cam), p->seed,
                                 plan.samples, p->max_depth, n_lights ? static_cast<const DLight*>(c->lights.p) : nullptr,
                                 n_lights, pass_light_grid(c), pass_light_sample(c),
                                 static_cast<const int32_t*>(c->prim_light.p), accum_dev, ad, c->cu_count,
                                 nee_blocks_cap(), s));
  return RT_OK;
}

int rt_render_nee_adaptive(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t flags,
                           const rt_adaptive_params* a, double* accum_host, int32_t* counts_host, double* moments_host,
                           double* tile_error_host, rt_adaptive_report* report) {
  int st = check_host_pass(c, cam);
  if (st) return st;
  if (!accum_host || !counts_host) return fail(c, RT_E_INVALID, "rt_render_nee_adaptive: an output buffer is NULL");
  const size_t n_px = (size_t)cam->image_width * cam->image_height;
  const int n_tiles = layout(cam, 0, (cam->image_height + kTile - 1) / kTile, 0, 1).n_tiles;
  // the errors come back in any case (the report counts them); the moments stay on the device when not asked for;
  // the counts, not doubles, follow the counter's word in a buffer of their own
  std::vector<double> err_own(tile_error_host ? 0 : n_tiles);
  double* err_host = tile_error_host ? tile_error_host : err_own.data();
  constexpr size_t kCountsAt = 64;
  if ((st = ensure(c, c->nee_adapt, kCountsAt + n_px * sizeof(int32_t)))) return st;
  if (!moments_host && (st = ensure(c, c->nee_moments, n_px * 2 * sizeof(double)))) return st;
  int32_t* counts_dev = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(c->nee_adapt.p) + kCountsAt);
  HostPlane pl[3] = {{accum_host, n_px * 3}, {moments_host, n_px * 2}, {err_host, (size_t)n_tiles}};
  st = pass_to_host(c, pl, 3, [&] {
    double* moments_dev = pl[1].dev ? pl[1].dev : static_cast<double*>(c->nee_moments.p);
    HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
    const int e = rt_render_nee_adaptive_device(c, cam, p, flags, a, pl[0].dev, counts_dev, moments_dev, pl[2].dev,
                                                c->stream);
    if (e) return e;
    HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(c, hipMemcpyAsync(counts_host, counts_dev, n_px * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return (int)RT_OK;
  });
  if (st) return st;
  if (report) {
    rt_adaptive_report rep{};
    int32_t most = a->min_samples;
    for (size_t i = 0; i < n_px; ++i) {
      rep.samples += (uint64_t)counts_host[i];
      most = std::max(most, counts_host[i]);
    }
    rep.steps = 1 + (int32_t)(((long long)most - a->min_samples + a->step - 1) / a->step);
    rep.tiles = n_tiles;
    for (int t = 0; t < n_tiles; ++t) rep.tiles_converged += err_host[t] <= a->threshold ? 1 : 0;
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    rep.kernel_ms = ms;  // (segments are not counted by this pass, and there is no fold: both stay 0)
    *report = rep;
  }
  return RT_OK;
}

}  // extern "C"
