// rt_direct.cpp — the light-list queries and the direct-lighting pass of include/shirley_rt.h (added within
// ABI 11; scene_compile.cpp list_lights, direct.hip).
#include "rt_ctx.h"

using namespace rt;

namespace {

int copy_lights(const std::vector<rt_light>& lights, int32_t n_unlisted, int32_t* n_lights, int32_t* n_out,
                rt_light* out) {
  if (n_lights) *n_lights = (int32_t)lights.size();
  if (n_out) *n_out = n_unlisted;
  if (out)
    for (size_t i = 0; i < lights.size(); ++i) out[i] = lights[i];
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_scene_lights(rt_ctx* c, int32_t* n_lights, int32_t* n_unlisted, rt_light* out) {
  if (!c) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "rt_scene_lights: no scene uploaded");
  return copy_lights(c->light_list, c->n_unlisted_lights, n_lights, n_unlisted, out);
}

int rt_scene_lights_host(const rt_scene_desc* d, int32_t* n_lights, int32_t* n_unlisted, rt_light* out) {
  if (!d || validate(d, nullptr)) return RT_E_INVALID;
  const LightList l = list_lights(d);
  return copy_lights(l.lights, l.n_unlisted, n_lights, n_unlisted, out);
}

int rt_render_direct_device(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t chain,
                            double* emission_dev, double* direct_dev, void* stream) {
  int st = pass_check(c, cam, p, "rt_render_direct");
  if (st) return st;
  if (chain < 0) return fail(c, RT_E_INVALID, "rt_render_direct: negative chain");
  if (!emission_dev && !direct_dev) return fail(c, RT_E_INVALID, "rt_render_direct: both output buffers are NULL");
  SampleRange R;
  hipStream_t s;
  if ((st = pass_begin(c, p, stream, "rt_render_direct", &R, &s))) return st;
  const int n_lights = (int)c->light_list.size();
  HIP_TRY(c, launch_direct(c->scene, c->place.wide, device_camera(cam), p->seed, R.begin, R.end, chain,
                           n_lights ? static_cast<const DLight*>(c->lights.p) : nullptr, n_lights,
                           pass_light_grid(c), pass_light_sample(c), emission_dev, direct_dev, s));
  return RT_OK;
}

int rt_render_direct(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t chain, double* emission_host,
                     double* direct_host) {
  const int st = check_host_pass(c, cam);
  if (st) return st;
  if (!emission_host && !direct_host) return fail(c, RT_E_INVALID, "rt_render_direct: both output buffers are NULL");
  const size_t n = (size_t)cam->image_width * cam->image_height * 3;
  HostPlane pl[2] = {{emission_host, n}, {direct_host, n}};
  return pass_to_host(c, pl, 2, [&] {
    return rt_render_direct_device(c, cam, p, chain, pl[0].dev, pl[1].dev, c->stream);
  });
}

}  // extern "C"
