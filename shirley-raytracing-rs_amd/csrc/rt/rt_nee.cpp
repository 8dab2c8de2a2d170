// rt_nee.cpp — the light-sampling path integrator of include/shirley_rt.h (added within ABI 11; nee.hip,
// direct.h).
#include "rt_ctx.h"

using namespace rt;

extern "C" {

int rt_render_nee_device(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t flags, double* accum_dev,
                         void* stream) {
  int st = check_render_args(c, cam, p);
  if (st) return st;
  if (flags & ~(int32_t)RT_NEE_MIS) return fail(c, RT_E_INVALID, "rt_render_nee: unknown flag bits 0x%x", flags);
  if (p->tile_world != 1) return fail(c, RT_E_INVALID, "rt_render_nee: tile_world must be 1");
  if (!accum_dev) return fail(c, RT_E_INVALID, "rt_render_nee: the output buffer is NULL");
  SampleRange R;
  if (resolve_range(c, p, &R)) return RT_E_INVALID;
  if (c->scene.exts) return fail(c, RT_E_UNSUPPORTED, "rt_render_nee: scenes with book-2 objects are not supported");
  hipStream_t s;
  resolve_stream(c, stream, &s);
  HIP_TRY(c, hipSetDevice(c->device));
  if (p->max_depth <= 0 || R.end <= R.begin) {  // no segment: zero sums
    const size_t n = (size_t)cam->image_width * cam->image_height * 3;
    HIP_TRY(c, hipMemsetAsync(accum_dev, 0, n * sizeof(double), s));
    return RT_OK;
  }
  const int n_lights = (int)c->light_list.size();
  HIP_TRY(c, launch_nee(c->scene, c->place.wide, (flags & RT_NEE_MIS) != 0, device_camera(cam), p->seed, R.begin, R.end,
                        p->max_depth, n_lights ? static_cast<const DLight*>(c->lights.p) : nullptr, n_lights,
                        static_cast<const int32_t*>(c->prim_light.p), accum_dev, s));
  return RT_OK;
}

int rt_render_nee(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t flags, double* accum_host) {
  if (!c) return RT_E_INVALID;
  if (!cam) return fail(c, RT_E_INVALID, "camera/params is NULL");
  if (cam->image_width < 1 || cam->image_height < 1) return fail(c, RT_E_INVALID, "bad image size");
  if (!accum_host) return fail(c, RT_E_INVALID, "rt_render_nee: the output buffer is NULL");
  const size_t n = (size_t)cam->image_width * cam->image_height * 3;
  int st = ensure(c, c->feat, n * sizeof(double));
  if (st) return st;
  double* acc = static_cast<double*>(c->feat.p);
  st = rt_render_nee_device(c, cam, p, flags, acc, c->stream);
  if (st) return st;
  HIP_TRY(c, hipMemcpyAsync(accum_host, acc, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

}  // extern "C"
