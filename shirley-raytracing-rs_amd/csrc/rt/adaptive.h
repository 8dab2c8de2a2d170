// adaptive.h — the rules of an adaptive frame (rt_render_adaptive): argument validation, the step
// schedule, the per-tile error and the stop rule (pure: no HIP, no context), so they can be checked on
// the CPU (tests/test_adaptive_plan.py via tools/adaptive_check).  fold_stats_kernel (trace.hip) applies
// the same pixel_variance / tile_error functions on the device.
//
// A batch is one work unit's samples (rt_render_params.sample_chunk, b of them): the trace kernel leaves
// one partial sum per (pixel, batch), y = (r + g) + b of it is one batch observation, and a pixel's
// moments are m1 = sum y, m2 = sum y^2 over its n batches so far.  For a tile of K in-image pixels after
// N = n b samples per pixel:
//   v_p = max(0, m2_p - m1_p^2 / n) / (n - 1)          batch-means variance of one batch sum
//   E = sum_p v_p,  M = sum_p m1_p
//   e = sqrt(n E / K) / (M / K + N noise_floor)
// n v_p estimates the variance of the pixel's sum m1_p, so sqrt(n E / K) is the RMS standard error of the
// tile's pixel sums and M / K their mean: e is the RMS standard error of the pixel means relative to the
// tile's mean r + g + b, with a floor so that dark tiles terminate.  A tile stops when e <= threshold (never
// at threshold 0); a NaN e (NaN radiance, or n = 1: no variance estimate) never does.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/shirley_rt.h"

#if defined(__HIPCC__)
#define RT_AD_FN __host__ __device__ inline
#else
#define RT_AD_FN inline
#endif

namespace rt {

constexpr int kAdaptiveDefaultBatch = 4;  // sample_chunk == 0

struct AdaptivePlan {
  int batch = 0;        // b: samples per batch (the unit length of every step)
  int min_samples = 0;  // step 0 renders [0, min_samples) of every pixel
  int step = 0;         // step k >= 1 renders [min_samples + (k - 1) step, min_samples + k step), clipped
  int samples = 0;      // the per-pixel maximum
  double threshold = 0.0, noise_floor = 0.0;
};

// nullptr when the call's arguments are valid (the plan is filled in), else what is wrong with them
inline const char* adaptive_validate(const rt_render_params* p, const rt_adaptive_params* a, AdaptivePlan* out) {
  if (!p || !a) return "params / adaptive params is NULL";
  if (p->sample_chunk < 0) return "negative sample_chunk";
  const int b = p->sample_chunk == 0 ? kAdaptiveDefaultBatch : p->sample_chunk;
  if (p->sample_begin != 0 || p->sample_count != 0) return "an adaptive frame takes no sample range (sample_begin / sample_count must be 0)";
  if (p->tile_world != 1 || p->tile_rank != 0) return "an adaptive frame is not tile-sharded (tile_world must be 1)";
  if (p->samples < 1 || p->samples % b != 0) return "samples must be a positive multiple of the batch (sample_chunk)";
  if (a->min_samples < 2 * b || a->min_samples % b != 0) return "min_samples must be a multiple of the batch and at least 2 batches";
  if (a->min_samples > p->samples) return "min_samples exceeds samples";
  if (a->step < b || a->step % b != 0) return "step must be a positive multiple of the batch";
  if (!(a->threshold >= 0.0)) return "threshold must be >= 0 (+inf allowed)";
  if (!(a->noise_floor >= 0.0) || !(a->noise_floor < HUGE_VAL)) return "noise_floor must be finite and >= 0";
  if (out) {
    out->batch = b;
    out->min_samples = a->min_samples;
    out->step = a->step;
    out->samples = p->samples;
    out->threshold = a->threshold;
    out->noise_floor = a->noise_floor;
  }
  return nullptr;
}

// steps of the schedule: [0, min), then [min + k step, min + (k + 1) step) clipped at samples
inline int adaptive_n_steps(const AdaptivePlan& P) {
  return 1 + (int)(((long long)P.samples - P.min_samples + P.step - 1) / P.step);
}
inline void adaptive_step_range(const AdaptivePlan& P, int k, int* begin, int* end) {
  if (k == 0) {
    *begin = 0;
    *end = P.min_samples;
    return;
  }
  const long long b = (long long)P.min_samples + (long long)(k - 1) * P.step;
  const long long e = b + P.step;
  *begin = (int)(b < P.samples ? b : P.samples);
  *end = (int)(e < P.samples ? e : P.samples);
}

// batch-means variance of one batch sum from a pixel's moments over n batches (NaN for n < 2; a NaN
// moment stays NaN)
RT_AD_FN double pixel_variance(double m1, double m2, long long n) {
  if (n < 2) return NAN;
  const double d = m2 - m1 * m1 / (double)n;
  return (d < 0.0 ? 0.0 : d) / (double)(n - 1);
}

// the tile's error from E = sum v_p and M = sum m1_p over its K in-image pixels, n batches of b samples
// per pixel.  A tile without variance (E == 0: e.g. all black) has e = 0 whatever its mean.
RT_AD_FN double tile_error(double E, double M, int K, long long n, int b, double noise_floor) {
  if (n < 2 || K < 1) return NAN;
  if (E == 0.0) return 0.0;
  const double N = (double)n * (double)b;
  return sqrt((double)n * E / (double)K) / (M / (double)K + N * noise_floor);
}

// the stop rule: a tile goes on while !(e <= threshold), so a NaN error keeps rendering; threshold 0 means
// never stop — also a tile without variance (e == 0), so that a threshold-0 frame is the uniform frame
RT_AD_FN bool tile_continues(double e, double threshold) { return !(e <= threshold) || threshold == 0.0; }

// the next step's list: the tiles of `list` (ascending global tile indices; err[i] is list[i]'s error)
// that go on, in the same order.  next may alias list.  Returns its length.
inline size_t adaptive_compact(const uint32_t* list, const double* err, size_t n, double threshold, uint32_t* next) {
  size_t m = 0;
  for (size_t i = 0; i < n; ++i)
    if (tile_continues(err[i], threshold)) next[m++] = list[i];
  return m;
}

}  // namespace rt
