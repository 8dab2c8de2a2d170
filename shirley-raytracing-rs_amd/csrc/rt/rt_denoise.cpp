// rt_denoise.cpp — the ABI 10 entry points of include/shirley_rt.h: the feature pass (features.hip) and the
// à-trous filter on the host (denoise.h's arithmetic, no device) and on the device (denoise.hip).
#include "denoise.h"
#include "rt_ctx.h"

using namespace rt;

extern "C" {

int rt_render_features_device(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t chain,
                              double* albedo_dev, double* normal_dev, double* depth_dev, void* stream) {
  int st = pass_check(c, cam, p, "rt_render_features");
  if (st) return st;
  if (chain < 0) return fail(c, RT_E_INVALID, "rt_render_features: negative chain");
  SampleRange R;
  hipStream_t s;
  if ((st = pass_range(c, p, "rt_render_features", &R))) return st;
  if (!albedo_dev && !normal_dev && !depth_dev) return RT_OK;  // (before the device is touched)
  if ((st = pass_device(c, stream, &s))) return st;
  HIP_TRY(c, launch_features(c->scene, c->place.wide, device_camera(cam), p->seed, R.begin, R.end, chain, albedo_dev,
                             normal_dev, depth_dev, s));
  return RT_OK;
}

int rt_render_features(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t chain, double* albedo_host,
                       double* normal_host, double* depth_host) {
  const int st = check_host_pass(c, cam);
  if (st) return st;
  const size_t n_px = (size_t)cam->image_width * cam->image_height;
  HostPlane pl[3] = {{albedo_host, n_px * 3}, {normal_host, n_px * 3}, {depth_host, n_px}};
  return pass_to_host(c, pl, 3, [&] {
    return rt_render_features_device(c, cam, p, chain, pl[0].dev, pl[1].dev, pl[2].dev, c->stream);
  });
}

int rt_denoise(const rt_denoise_inputs* in, const rt_denoise_params* prm, double* out) {
  return denoise_host(in, prm, out) ? RT_E_INVALID : RT_OK;
}

int rt_denoise_device(rt_ctx* c, const rt_denoise_inputs* in, const rt_denoise_params* prm, double* out_dev,
                      void* stream) {
  if (!c) return RT_E_INVALID;
  if (const char* why = denoise_validate(in, prm)) return fail(c, RT_E_INVALID, "rt_denoise_device: %s", why);
  if (!out_dev) return fail(c, RT_E_INVALID, "rt_denoise_device: out_sums_dev is NULL");
  hipStream_t s;
  resolve_stream(c, stream, &s);
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n_px = (size_t)in->width * in->height;
  if (prm->iterations == 0) {
    HIP_TRY(c, hipMemcpyAsync(out_dev, in->accum, n_px * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    return RT_OK;
  }
  int st;
  if ((st = ensure(c, c->dn_a, n_px * kDnRecord * sizeof(double))) ||
      (st = ensure(c, c->dn_b, n_px * kDnRecord * sizeof(double))))
    return st;
  HIP_TRY(c, launch_denoise(*in, *prm, static_cast<double*>(c->dn_a.p), static_cast<double*>(c->dn_b.p), out_dev, s));
  return RT_OK;
}

int rt_moments_variance(const double* moments, const int32_t* counts, int32_t batch, int32_t width, int32_t height,
                        double* out) {
  if (!moments || !counts || !out || batch < 1 || width < 1 || height < 1) return RT_E_INVALID;
  const size_t n_px = (size_t)width * height;
  for (size_t i = 0; i < n_px; ++i) {
    if (counts[i] < 0) return RT_E_INVALID;
    out[i] = dn_moments_variance(moments[i * 2], moments[i * 2 + 1], counts[i], batch);
  }
  return RT_OK;
}

int rt_moments_variance_device(rt_ctx* c, const double* moments_dev, const int32_t* counts_dev, int32_t batch,
                               int32_t width, int32_t height, double* out_dev, void* stream) {
  if (!c) return RT_E_INVALID;
  if (!moments_dev || !counts_dev || !out_dev || batch < 1 || width < 1 || height < 1)
    return fail(c, RT_E_INVALID, "rt_moments_variance_device: bad argument");
  hipStream_t s;
  resolve_stream(c, stream, &s);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, launch_moments_variance(moments_dev, counts_dev, batch, (long long)width * height, out_dev, s));
  return RT_OK;
}

}  // extern "C"
