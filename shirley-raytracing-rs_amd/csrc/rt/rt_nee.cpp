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

}  // extern "C"
