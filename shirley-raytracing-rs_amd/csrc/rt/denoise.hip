// denoise.hip — the à-trous filter's kernels (rt_denoise_device, rt_moments_variance_device): dn_prepare
// packs every pixel's demodulated colour, variance, albedo, depth, normal and live flag into one 96-byte
// record, dn_atrous runs one iteration from one record buffer into the other, dn_finish re-modulates.  The
// arithmetic is denoise.h's, the functions the host's rt_denoise calls: the results are bit-identical.
//
// One thread per pixel; each wave covers an 8x8 tile (lane l = pixel (l % 8, l / 8) of it), so the 25 taps
// of neighbouring lanes fall into the same few cache lines: a tap row of a wave at stride 1 spans 12
// records, 9 cache lines of 128 B.  No LDS tile: the records of a 5x5 neighbourhood are read through L1 / L2.
#include <hip/hip_runtime.h>

#include "denoise.h"
#include "rt_launch.h"
#include "rt_layout.h"

namespace rt {

constexpr int kDnThreads = 256;  // 4 waves = 4 tiles per block

struct DnPixel {
  int x, y;
  bool in;
};
__device__ __forceinline__ DnPixel dn_pixel(int width, int height, int tiles_x, int n_tiles) {
  const int tile = blockIdx.x * (kDnThreads / kWave) + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  DnPixel p;
  p.x = (tile % tiles_x) * kTile + lane % kTile;
  p.y = (tile / tiles_x) * kTile + lane / kTile;
  p.in = tile < n_tiles && p.x < width && p.y < height;
  return p;
}

__global__ __launch_bounds__(kDnThreads) void dn_prepare(const double* __restrict__ accum,
                                                         const int32_t* __restrict__ counts, int samples,
                                                         const double* __restrict__ albedo,
                                                         const double* __restrict__ normal,
                                                         const double* __restrict__ depth,
                                                         const double* __restrict__ variance, int feature_samples,
                                                         double floor_, int width, int height, int tiles_x,
                                                         int n_tiles, double* __restrict__ recs) {
  const DnPixel p = dn_pixel(width, height, tiles_x, n_tiles);
  if (!p.in) return;
  const size_t i = (size_t)p.y * width + p.x;
  double rec[kDnRecord];
  dn_prepare_pixel(accum + i * 3, counts ? counts[i] : samples, albedo + i * 3, normal + i * 3, depth[i],
                   variance ? variance[i] : 0.0, variance != nullptr, feature_samples, floor_, rec);
#pragma unroll
  for (int k = 0; k < kDnRecord; ++k) recs[i * kDnRecord + k] = rec[k];
}

__global__ __launch_bounds__(kDnThreads) void dn_atrous(const double* __restrict__ in, int width, int height,
                                                        int tiles_x, int n_tiles, int stride, rt_denoise_params prm,
                                                        int has_var, double* __restrict__ out) {
  const DnPixel p = dn_pixel(width, height, tiles_x, n_tiles);
  if (!p.in) return;
  double rec[kDnRecord];
  dn_atrous_pixel(in, width, height, p.x, p.y, stride, prm, has_var != 0, rec);
  const size_t i = (size_t)p.y * width + p.x;
#pragma unroll
  for (int k = 0; k < kDnRecord; ++k) out[i * kDnRecord + k] = rec[k];
}

__global__ __launch_bounds__(kDnThreads) void dn_finish(const double* __restrict__ recs,
                                                        const int32_t* __restrict__ counts, int samples,
                                                        double floor_, int width, int height, int tiles_x,
                                                        int n_tiles, double* __restrict__ out) {
  const DnPixel p = dn_pixel(width, height, tiles_x, n_tiles);
  if (!p.in) return;
  const size_t i = (size_t)p.y * width + p.x;
  double o[3];
  dn_finish_pixel(recs + i * kDnRecord, counts ? counts[i] : samples, floor_, o);
  out[i * 3 + 0] = o[0];
  out[i * 3 + 1] = o[1];
  out[i * 3 + 2] = o[2];
}

__global__ __launch_bounds__(256) void dn_moments_variance_kernel(const double* __restrict__ moments,
                                                                  const int32_t* __restrict__ counts, int batch,
                                                                  long long n, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = dn_moments_variance(moments[i * 2], moments[i * 2 + 1], counts[i], batch);
}

// the whole filter on `stream`: recs_a / recs_b are [H][W][kDnRecord] scratch; iterations >= 1 (the caller
// copies the input for 0)
hipError_t launch_denoise(const rt_denoise_inputs& in, const rt_denoise_params& prm, double* recs_a, double* recs_b,
                          double* out, hipStream_t stream) {
  const int tiles_x = (in.width + kTile - 1) / kTile, tiles_y = (in.height + kTile - 1) / kTile;
  const int n_tiles = tiles_x * tiles_y;
  const int per_block = kDnThreads / kWave;
  const int blocks = (n_tiles + per_block - 1) / per_block;
  hipLaunchKernelGGL(dn_prepare, dim3(blocks), dim3(kDnThreads), 0, stream, in.accum, in.counts, in.samples, in.albedo,
                     in.normal, in.depth, in.variance, in.feature_samples, prm.albedo_floor, in.width, in.height,
                     tiles_x, n_tiles, recs_a);
  double *src = recs_a, *dst = recs_b;
  for (int i = 0; i < prm.iterations; ++i) {
    hipLaunchKernelGGL(dn_atrous, dim3(blocks), dim3(kDnThreads), 0, stream, src, in.width, in.height, tiles_x, n_tiles,
                       1 << i, prm, in.variance != nullptr ? 1 : 0, dst);
    double* t = src;
    src = dst;
    dst = t;
  }
  hipLaunchKernelGGL(dn_finish, dim3(blocks), dim3(kDnThreads), 0, stream, src, in.counts, in.samples,
                     prm.albedo_floor, in.width, in.height, tiles_x, n_tiles, out);
  return hipGetLastError();
}

hipError_t launch_moments_variance(const double* moments, const int32_t* counts, int batch, long long n, double* out,
                                   hipStream_t stream) {
  const long long blocks = (n + 255) / 256;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(dn_moments_variance_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, moments, counts, batch,
                     n, out);
  return hipGetLastError();
}

}  // namespace rt
