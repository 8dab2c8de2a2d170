// rt_denoise.cpp — the ABI 10 entry points of include/shirley_rt.h: the feature pass (features.hip) and the
// à-trous filter on the host (denoise.h's arithmetic, no device) and on the device (denoise.hip).
#include "denoise.h"
#include "rt_ctx.h"

using namespace rt;

extern "C" {

int rt_render_features_device(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t chain,
                              double* albedo_dev, double* normal_dev, double* depth_dev, void* stream) {
  int st = check_render_args(c, cam, p);
  if (st) return st;
  if (p->tile_world != 1) return fail(c, RT_E_INVALID, "rt_render_features: tile_world must be 1");
  if (chain < 0) return fail(c, RT_E_INVALID, "rt_render_features: negative chain");
  SampleRange R;
  if (resolve_range(c, p, &R)) return RT_E_INVALID;
  if (c->scene.exts)
    return fail(c, RT_E_UNSUPPORTED, "rt_render_features: scenes with book-2 objects are not supported");
  if (!albedo_dev && !normal_dev && !depth_dev) return RT_OK;
  hipStream_t s;
  resolve_stream(c, stream, &s);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, launch_features(c->scene, c->place.wide, device_camera(cam), p->seed, R.begin, R.end, chain, albedo_dev,
                             normal_dev, depth_dev, s));
  return RT_OK;
}

int rt_render_features(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int32_t chain, double* albedo_host,
                       double* normal_host, double* depth_host) {
  if (!c) return RT_E_INVALID;
  if (!cam) return fail(c, RT_E_INVALID, "camera/params is NULL");
  if (cam->image_width < 1 || cam->image_height < 1) return fail(c, RT_E_INVALID, "bad image size");
  const size_t n_px = (size_t)cam->image_width * cam->image_height;
  int st = ensure(c, c->feat, n_px * 7 * sizeof(double));
  if (st) return st;
  double* base = static_cast<double*>(c->feat.p);
  double* a = albedo_host ? base : nullptr;
  double* n = normal_host ? base + n_px * 3 : nullptr;
  double* z = depth_host ? base + n_px * 6 : nullptr;
  st = rt_render_features_device(c, cam, p, chain, a, n, z, c->stream);
  if (st) return st;
  if (a) HIP_TRY(c, hipMemcpyAsync(albedo_host, a, n_px * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (n) HIP_TRY(c, hipMemcpyAsync(normal_host, n, n_px * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (z) HIP_TRY(c, hipMemcpyAsync(depth_host, z, n_px * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return RT_OK;
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
