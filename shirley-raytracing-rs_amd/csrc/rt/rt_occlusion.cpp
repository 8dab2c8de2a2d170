// rt_occlusion.cpp — the ABI 11 entry points of include/shirley_rt.h: the batch occlusion query and the
// ambient-occlusion pass (occlusion.hip).
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rt_ctx.h"

using namespace rt;

namespace {

// The instance rt_scene_occluded answers through: the any-hit walk (occluded4) on every placement — on neither
// measured batch was it slower than traverse4 beyond the run-to-run spread.
// SHIRLEY_OCCLUDED_CLOSEST=1 selects the traverse4 instance (measurement, cross-check); read at the call.
bool occluded_closest() {
  const char* e = getenv("SHIRLEY_OCCLUDED_CLOSEST");
  return e && !strcmp(e, "1");
}

int check_occluded_args(rt_ctx* c, const double* rays, int32_t n, double t_min, double t_max, const uint8_t* out) {
  if (!c) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "rt_scene_occluded: no scene uploaded");
  if (n < 0 || !rays || !out) return fail(c, RT_E_INVALID, "rt_scene_occluded: bad ray batch");
  if (std::isnan(t_min) || std::isnan(t_max)) return fail(c, RT_E_INVALID, "rt_scene_occluded: t_min / t_max is NaN");
  if (c->scene.exts)
    return fail(c, RT_E_UNSUPPORTED, "rt_scene_occluded: scenes with book-2 objects are not supported");
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_scene_occluded_device(rt_ctx* c, const double* rays_dev, int32_t n, double t_min, double t_max,
                             const double* t_max_each_dev, uint8_t* out_dev, void* stream) {
  int st = check_occluded_args(c, rays_dev, n, t_min, t_max, out_dev);
  if (st) return st;
  if (n == 0) return RT_OK;
  hipStream_t s;
  resolve_stream(c, stream, &s);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, launch_occluded(c->scene, c->place.wide, occluded_closest(), rays_dev, n, t_min, t_max, t_max_each_dev,
                             out_dev, s));
  return RT_OK;
}

int rt_scene_occluded(rt_ctx* c, const double* rays, int32_t n, double t_min, double t_max, const double* t_max_each,
                      uint8_t* out) {
  int st = check_occluded_args(c, rays, n, t_min, t_max, out);
  if (st) return st;
  if (n == 0) return RT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  DevBuf r, t, o;
  st = upload(c, r, rays, (size_t)n * 6 * sizeof(double));
  if (!st && t_max_each) st = upload(c, t, t_max_each, (size_t)n * sizeof(double));
  if (!st) st = ensure(c, o, (size_t)n);
  if (!st) st = rt_scene_occluded_device(c, static_cast<const double*>(r.p), n, t_min, t_max,
                                         t_max_each ? static_cast<const double*>(t.p) : nullptr,
                                         static_cast<uint8_t*>(o.p), c->stream);
  if (!st) {
    hipError_t e = hipMemcpyAsync(out, o.p, (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) st = fail(c, RT_E_HIP, "rt_scene_occluded: %s", hipGetErrorString(e));
  }
  release(r);
  release(t);
  release(o);
  return st;
}

int rt_render_ao_device(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t chain, double radius,
                        double* ao_dev, void* stream) {
  int st = pass_check(c, cam, p, "rt_render_ao");
  if (st) return st;
  if (chain < 0) return fail(c, RT_E_INVALID, "rt_render_ao: negative chain");
  if (!(radius > 0.0)) return fail(c, RT_E_INVALID, "rt_render_ao: radius must be > 0 (or +inf)");
  if (!ao_dev) return fail(c, RT_E_INVALID, "rt_render_ao: the output buffer is NULL");
  SampleRange R;
  hipStream_t s;
  if ((st = pass_begin(c, p, stream, "rt_render_ao", &R, &s))) return st;
  HIP_TRY(c, launch_ao(c->scene, c->place.wide, device_camera(cam), p->seed, R.begin, R.end, chain, radius, ao_dev, s));
  return RT_OK;
}

int rt_render_ao(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t chain, double radius,
                 double* ao_host) {
  const int st = check_host_pass(c, cam);
  if (st) return st;
  if (!ao_host) return fail(c, RT_E_INVALID, "rt_render_ao: the output buffer is NULL");
  HostPlane pl{ao_host, (size_t)cam->image_width * cam->image_height};
  return pass_to_host(c, &pl, 1, [&] { return rt_render_ao_device(c, cam, p, chain, radius, pl.dev, c->stream); });
}

}  // extern "C"
