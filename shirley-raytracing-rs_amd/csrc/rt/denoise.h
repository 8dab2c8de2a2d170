// denoise.h — the arithmetic of the edge-aware à-trous filter (rt_denoise / rt_denoise_device): the
// argument rules, the per-pixel prepare / finish steps, the edge-stopping weights and the 5x5 tap loop
// (pure: no HIP, no context), shared by the host function (rt_denoise.cpp) and the kernels (denoise.hip) so
// that both run the same operations in the same order.  Only + - * /, comparisons and selects: no libm
// and no fused multiply-add (both sides are built with -ffp-contract=off), so the device result equals
// the host's bit for bit and a numpy restatement is exact (tests/test_denoise.py, tools/denoise_check).
//
// With c, a, n, z the per-pixel means of the frame, albedo, normal and depth (sums / counts):
//   prepare   c^ = c / max(a, floor) per channel; var^ = var / ((A0^2 + A1^2 + A2^2) / 3), A = max(a, floor)
//   iteration i = 0 .. iterations-1, stride s = 2^i, taps (dy, dx) in -2..2 (dy outer), offsets s (dx, dy):
//               c^'_p = sum_q h_q w_pq c^_q / sum_q h_q w_pq,  var^'_p = sum_q (h_q w_pq)^2 var^_q / (sum_q h_q w_pq)^2
//               h = (1/16, 1/4, 3/8, 1/4, 1/16) x itself; w_pp = 1; w_pq = ((w_n w_z) w_a) w_c, f(x) = max(0, 1 - x)^2
//   finish    out = (c^ max(a, floor)) count
// A record is one pixel's state, 12 doubles: c^[3], var^, a[3], z, n[3], live (1: count > 0).  A pixel that is
// not live (count 0) or whose c^ is not finite is copied through an iteration unchanged and is skipped as a
// neighbour.
#pragma once

#include <utility>
#include <vector>

#include "adaptive.h"

namespace rt {

constexpr int kDnRecord = 12;  // doubles per pixel record
enum : int { kDnC = 0, kDnVar = 3, kDnA = 4, kDnZ = 7, kDnN = 8, kDnLive = 11 };
constexpr int kDnMaxIterations = 8;
constexpr int kDnMaxNormalPower = 16;

// nullptr when the call's arguments are valid, else what is wrong with them (the per-pixel counts are
// checked by denoise_host)
inline const char* denoise_validate(const rt_denoise_inputs* in, const rt_denoise_params* p) {
  if (!in || !p) return "inputs / params is NULL";
  if (in->width < 1 || in->height < 1 || in->width > (1 << 16) || in->height > (1 << 16)) return "bad image size";
  if (!in->accum || !in->albedo || !in->normal || !in->depth) return "accum / albedo / normal / depth is NULL";
  if (!in->counts && in->samples < 1) return "samples must be >= 1 (or pass counts)";
  if (in->feature_samples < 1) return "feature_samples must be >= 1";
  if (p->iterations < 0 || p->iterations > kDnMaxIterations) return "iterations must be in [0, 8]";
  if (p->normal_power_log2 < 0 || p->normal_power_log2 > kDnMaxNormalPower) return "normal_power_log2 must be in [0, 16]";
  if (!(p->sigma_z > 0.0) || !(p->sigma_a > 0.0) || !(p->sigma_c > 0.0)) return "sigma_z, sigma_a, sigma_c must be > 0";
  if (!(p->albedo_floor > 0.0)) return "albedo_floor must be > 0";
  return nullptr;
}

RT_AD_FN double dn_max(double a, double b) { return a > b ? a : b; }
RT_AD_FN bool dn_finite(double x) { return x - x == 0.0; }
RT_AD_FN double dn_f(double x) {
  const double t = dn_max(0.0, 1.0 - x);
  return t * t;
}

// one pixel's record from its sums (var: the variance of the mean r + g + b, ignored when !has_var)
RT_AD_FN void dn_prepare_pixel(const double* accum3, int count, const double* albedo3, const double* normal3,
                               double depth, double var, bool has_var, int feature_samples, double floor_,
                               double* rec) {
  const double fs = (double)feature_samples;
  const double a0 = albedo3[0] / fs, a1 = albedo3[1] / fs, a2 = albedo3[2] / fs;
  const double A0 = dn_max(a0, floor_), A1 = dn_max(a1, floor_), A2 = dn_max(a2, floor_);
  const bool live = count > 0;
  const double n = (double)count;
  rec[kDnC + 0] = live ? (accum3[0] / n) / A0 : 0.0;
  rec[kDnC + 1] = live ? (accum3[1] / n) / A1 : 0.0;
  rec[kDnC + 2] = live ? (accum3[2] / n) / A2 : 0.0;
  rec[kDnVar] = (has_var && live) ? var / (((A0 * A0 + A1 * A1) + A2 * A2) / 3.0) : 0.0;
  rec[kDnA + 0] = a0;
  rec[kDnA + 1] = a1;
  rec[kDnA + 2] = a2;
  rec[kDnZ] = depth / fs;
  rec[kDnN + 0] = normal3[0] / fs;
  rec[kDnN + 1] = normal3[1] / fs;
  rec[kDnN + 2] = normal3[2] / fs;
  rec[kDnLive] = live ? 1.0 : 0.0;
}

RT_AD_FN bool dn_usable(const double* rec) {
  return rec[kDnLive] != 0.0 && dn_finite(rec[kDnC + 0]) && dn_finite(rec[kDnC + 1]) && dn_finite(rec[kDnC + 2]);
}

// w_pq for q != p
RT_AD_FN double dn_weight(const double* P, const double* Q, double nn_p, const rt_denoise_params& prm, bool has_var) {
  const double nn_q = (Q[kDnN] * Q[kDnN] + Q[kDnN + 1] * Q[kDnN + 1]) + Q[kDnN + 2] * Q[kDnN + 2];
  double wn;
  if (nn_p == 0.0 && nn_q == 0.0) {
    wn = 1.0;  // both sky
  } else if (nn_p == 0.0 || nn_q == 0.0) {
    wn = 0.0;
  } else {
    const double d = dn_max(0.0, (P[kDnN] * Q[kDnN] + P[kDnN + 1] * Q[kDnN + 1]) + P[kDnN + 2] * Q[kDnN + 2]);
    wn = (d * d) / (nn_p * nn_q);
    for (int k = 0; k < prm.normal_power_log2; ++k) wn = wn * wn;
  }
  const double r = (P[kDnZ] - Q[kDnZ]) / (prm.sigma_z * (P[kDnZ] + Q[kDnZ]) + 1e-300);
  const double wz = dn_f(r * r);
  const double ax = P[kDnA] - Q[kDnA], ay = P[kDnA + 1] - Q[kDnA + 1], az = P[kDnA + 2] - Q[kDnA + 2];
  const double wa = dn_f(((ax * ax + ay * ay) + az * az) / (prm.sigma_a * prm.sigma_a));
  double w = (wn * wz) * wa;
  if (has_var) {
    const double cx = P[kDnC] - Q[kDnC], cy = P[kDnC + 1] - Q[kDnC + 1], cz = P[kDnC + 2] - Q[kDnC + 2];
    const double wc = dn_f(((cx * cx + cy * cy) + cz * cz) /
                           ((prm.sigma_c * prm.sigma_c) * (P[kDnVar] + Q[kDnVar]) + 1e-300));
    w = w * wc;
  }
  return w;
}

// one iteration for pixel (x, y): reads records of `in` ([H][W][kDnRecord]), writes the pixel's record to `out`
RT_AD_FN void dn_atrous_pixel(const double* in, int width, int height, int x, int y, int stride,
                              const rt_denoise_params& prm, bool has_var, double* out) {
  const double kh[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
  const double* P = in + ((size_t)y * width + x) * kDnRecord;
  for (int k = 0; k < kDnRecord; ++k) out[k] = P[k];
  if (!dn_usable(P)) return;
  const double nn_p = (P[kDnN] * P[kDnN] + P[kDnN + 1] * P[kDnN + 1]) + P[kDnN + 2] * P[kDnN + 2];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, sw = 0.0, sv = 0.0;
  for (int dy = -2; dy <= 2; ++dy) {
    const long long qy = (long long)y + (long long)dy * stride;
    if (qy < 0 || qy >= height) continue;
    for (int dx = -2; dx <= 2; ++dx) {
      const long long qx = (long long)x + (long long)dx * stride;
      if (qx < 0 || qx >= width) continue;
      const double* Q = in + ((size_t)qy * width + (size_t)qx) * kDnRecord;
      double w = 1.0;
      if (dx != 0 || dy != 0) {
        if (!dn_usable(Q)) continue;
        w = dn_weight(P, Q, nn_p, prm, has_var);
      }
      const double hw = (kh[dy + 2] * kh[dx + 2]) * w;
      s0 += hw * Q[kDnC + 0];
      s1 += hw * Q[kDnC + 1];
      s2 += hw * Q[kDnC + 2];
      sw += hw;
      sv += (hw * hw) * Q[kDnVar];
    }
  }
  out[kDnC + 0] = s0 / sw;
  out[kDnC + 1] = s1 / sw;
  out[kDnC + 2] = s2 / sw;
  out[kDnVar] = sv / (sw * sw);
}

// the pixel's output sums from its record
RT_AD_FN void dn_finish_pixel(const double* rec, int count, double floor_, double* out3) {
  const double n = (double)count;
  for (int k = 0; k < 3; ++k)
    out3[k] = count > 0 ? (rec[kDnC + k] * dn_max(rec[kDnA + k], floor_)) * n : 0.0;
}

// rt_moments_variance for one pixel: the variance of the mean r + g + b of a pixel that holds `count`
// samples in batches of `batch` (adaptive.h: v_p is the batch-means variance of one batch sum, n v_p that of
// the pixel's sum, N = count samples).  NaN for fewer than two batches.
RT_AD_FN double dn_moments_variance(double m1, double m2, int count, int batch) {
  const long long n = count / batch;
  const double N = (double)count;
  return (pixel_variance(m1, m2, n) * (double)n) / (N * N);
}

// the whole filter on the host (rt_denoise; tools/denoise_check): nullptr, or what is wrong with the arguments
inline const char* denoise_host(const rt_denoise_inputs* in, const rt_denoise_params* prm, double* out) {
  if (const char* why = denoise_validate(in, prm)) return why;
  if (!out) return "out_sums is NULL";
  const int W = in->width, H = in->height;
  const size_t n_px = (size_t)W * H;
  if (in->counts)
    for (size_t i = 0; i < n_px; ++i)
      if (in->counts[i] < 0) return "negative count";
  if (prm->iterations == 0) {
    for (size_t i = 0; i < n_px * 3; ++i) out[i] = in->accum[i];
    return nullptr;
  }
  const bool has_var = in->variance != nullptr;
  std::vector<double> a(n_px * kDnRecord), b(n_px * kDnRecord);
  for (size_t i = 0; i < n_px; ++i)
    dn_prepare_pixel(in->accum + i * 3, in->counts ? in->counts[i] : in->samples, in->albedo + i * 3,
                     in->normal + i * 3, in->depth[i], has_var ? in->variance[i] : 0.0, has_var, in->feature_samples,
                     prm->albedo_floor, &a[i * kDnRecord]);
  double *src = a.data(), *dst = b.data();
  for (int it = 0; it < prm->iterations; ++it) {
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        dn_atrous_pixel(src, W, H, x, y, 1 << it, *prm, has_var, dst + ((size_t)y * W + x) * kDnRecord);
    std::swap(src, dst);
  }
  for (size_t i = 0; i < n_px; ++i)
    dn_finish_pixel(src + i * kDnRecord, in->counts ? in->counts[i] : in->samples, prm->albedo_floor, out + i * 3);
  return nullptr;
}

}  // namespace rt
