// occlusion.hip — rt_scene_occluded and rt_render_ao (include/shirley_rt.h, ABI 11).
//
// occluded_kernel: one ray per lane in the manner of hit4_kernel (trace.hip) — the same MODE staging of nodes
// and primitives and the same LDS sizing — answering through the any-hit walk occluded4 (occlusion.h) or,
// in its second instance (CLOSEST), through traverse4 (`best >= 0`); both give the same bytes.
// ao_kernel: modelled on features_kernel (features.hip) — one wave per 8x8 tile, one lane per pixel, the
// sample loop inside the lane, the same camera ray and dielectric chain — without a texture, so without the
// wave-wide marble: lanes outside the image leave after the staging.  At the feature vertex it forms the
// renderer's Lambertian scatter direction on the path's own draws and asks occluded4 along it.
// Reference scenes only (no book-2 records): EXT = false instances.
#include <hip/hip_runtime.h>

#include "occlusion.h"
#include "rt_launch.h"

namespace rt {

// Block of the scene-in-LDS placements (`wide`), as features.hip's: the megakernel's 1024 threads, which the
// placement plan sized the LDS stacks for.
constexpr int kOccThreadsWide = kTraceThreadsWide;

template <int MODE>
__device__ __forceinline__ unsigned* occ_lds_carve(const DScene& S, unsigned char* lds_raw, DNode4F*& lds_nodes,
                                                   DPrim*& lds_prims) {
  lds_nodes = reinterpret_cast<DNode4F*>(lds_raw);
  lds_prims = reinterpret_cast<DPrim*>(lds_raw + (size_t)S.n_lds_nodes4 * sizeof(DNode4F));
  unsigned char* stk_base = lds_raw + (size_t)S.n_lds_nodes4 * sizeof(DNode4F) +
                            (MODE == kSceneLds ? (size_t)S.n_lds_prims * sizeof(DPrim) +
                                                     (size_t)S.n_lds_perlin * sizeof(DPerlin) +
                                                     (size_t)S.n_lds_mats * sizeof(DMat) +
                                                     (size_t)S.n_lds_texs * sizeof(DTex)
                                               : 0);
  return reinterpret_cast<unsigned*>(stk_base) + threadIdx.x;
}

template <int THREADS, int MODE, bool CLOSEST>
__global__ __launch_bounds__(THREADS) void occluded_kernel(DScene S, const double* __restrict__ rays, int n,
                                                           double t_min, double t_max,
                                                           const double* __restrict__ t_max_each,
                                                           uint8_t* __restrict__ out) {
  extern __shared__ unsigned char lds_raw[];
  DNode4F* lds_nodes;
  DPrim* lds_prims;
  unsigned* stk = occ_lds_carve<MODE>(S, lds_raw, lds_nodes, lds_prims);
  stage_nodes4<MODE>(S, lds_nodes, lds_prims);
  const int i = blockIdx.x * THREADS + (int)threadIdx.x;
  if (i >= n) return;
  const double* r = rays + (size_t)i * 6;
  const v3 o = V(r[0], r[1], r[2]);
  const v3 d = V(r[3], r[4], r[5]);
  const double tm = t_max_each ? t_max_each[i] : t_max;
  unsigned visits = 0, ptests = 0;
  bool occ;
  if constexpr (CLOSEST) {
    double t_best = tm;
    int face = -1;
    const Rng rk{(uint32_t)i, 0u, 0u, 0u, 0u};
#ifdef RT_PHASE_TIMING
    unsigned long long steps = 0;
#endif
    occ = traverse4<THREADS, MODE, false>(S, lds_nodes, lds_prims, o, d, t_min, t_best, face, stk, rk, 0ull, visits,
                                          ptests RT_STAT_ARG(steps)) >= 0;
  } else {
    occ = occluded4<THREADS, MODE>(S, lds_nodes, lds_prims, o, d, t_min, tm, stk, visits, ptests);
  }
  out[i] = occ ? 1 : 0;
}

template <int THREADS, int MODE>
__global__ __launch_bounds__(THREADS) void ao_kernel(DScene S, DCamera C, uint64_t seed, int s_begin, int s_end,
                                                     int chain, double radius, int tiles_x, int n_tiles,
                                                     double* __restrict__ ao) {
  extern __shared__ unsigned char lds_raw[];
  DNode4F* lds_nodes;
  DPrim* lds_prims;
  unsigned* stk = occ_lds_carve<MODE>(S, lds_raw, lds_nodes, lds_prims);
  stage_nodes4<MODE>(S, lds_nodes, lds_prims);
  // wave w of the block renders tile blockIdx * (THREADS / 64) + w; lane l its pixel (l % 8, l / 8)
  const int tid = threadIdx.x;
  const int tile = blockIdx.x * (THREADS / kWave) + tid / kWave;
  const int lane = tid % kWave;
  const int px = (tile % tiles_x) * kTile + lane % kTile;
  const int py = (tile / tiles_x) * kTile + lane / kTile;
  if (tile >= n_tiles || px >= C.width || py >= C.height) return;  // (nothing wave-wide follows)
  const uint32_t pix = (uint32_t)py * (uint32_t)C.width + (uint32_t)px;
  double sum = 0.0;
  unsigned visits = 0, ptests = 0;
#ifdef RT_PHASE_TIMING
  unsigned long long steps = 0;
#endif
  for (int s = s_begin; s < s_end; ++s) {
    Rng rng{pix, (uint32_t)s, 0u, 0u, 0u};
    v3 o, d;
    const double jx = (double)px + rng_next(rng, seed);  // render.rs:60-63
    const double jy = (double)py + rng_next(rng, seed);
    camera_ray(C, rng, seed, jx, jy, o, d);
    Hit h;
    bool hit;
    int left = chain;
    for (;;) {  // features_kernel's walk to the feature vertex
      double t_best = __builtin_inf();
      int face = -1;
      const int prim = traverse4<THREADS, MODE, false>(S, lds_nodes, lds_prims, o, d, 0.001, t_best, face, stk, rng,
                                                       seed, visits, ptests RT_STAT_ARG(steps));
      hit = prim >= 0;
      if (!hit) break;
      const DPrim pr = (MODE == kSceneLds) ? lds_prims[prim] : S.prims[prim];
      hit_record<false, false>(S, pr, face, o, d, t_best, rng, seed, h);
      const DMat& m = S.mats[pr.material];
      if (m.kind != RT_MAT_DIELECTRIC || left <= 0) break;
      --left;
      const v3 rs = draw_diel(rng, seed);
      shade_dielectric(m, rs, unit_fast(d), rng, o, d, h);
    }
    if (!hit) {  // a miss sees the sky
      sum += 1.0;
      continue;
    }
    // the renderer's Lambertian scatter at the record (shade(): lambertian.rs:21-37), whatever the material
    const v3 r = random_in_unit_sphere(rng, seed);
    v3 w = h.normal + unit(r);
    if (near_zero(w)) w = h.normal;
    const double t_max = radius / len(w);
    sum += occluded4<THREADS, MODE>(S, lds_nodes, lds_prims, h.point, w, 0.001, t_max, stk, visits, ptests) ? 0.0 : 1.0;
  }
  ao[(size_t)py * (size_t)C.width + (size_t)px] = sum;
}

template <int THREADS, int MODE>
static size_t occ_lds_bytes(const DScene& S) {
  return trace_lds_bytes(S.n_lds_nodes4, node4_bytes(false), MODE == kSceneLds ? S.n_lds_prims : 0,
                         MODE == kSceneLds ? S.n_lds_perlin : 0, S.stack_depth4, THREADS,
                         MODE == kSceneLds ? S.n_lds_mats : 0, MODE == kSceneLds ? S.n_lds_texs : 0);
}

template <int THREADS, int MODE, bool CLOSEST>
static hipError_t launch_occluded_2(const DScene& S, const double* rays, int n, double t_min, double t_max,
                                    const double* t_max_each, uint8_t* out, hipStream_t stream) {
  const size_t lds = occ_lds_bytes<THREADS, MODE>(S);
  hipError_t e = hipFuncSetAttribute((const void*)occluded_kernel<THREADS, MODE, CLOSEST>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  const int blocks = (n + THREADS - 1) / THREADS;
  hipLaunchKernelGGL((occluded_kernel<THREADS, MODE, CLOSEST>), dim3(blocks), dim3(THREADS), lds, stream, S, rays, n,
                     t_min, t_max, t_max_each, out);
  return hipGetLastError();
}
template <int THREADS, int MODE>
static hipError_t launch_occluded_1(const DScene& S, bool closest, const double* rays, int n, double t_min,
                                    double t_max, const double* t_max_each, uint8_t* out, hipStream_t stream) {
  return closest ? launch_occluded_2<THREADS, MODE, true>(S, rays, n, t_min, t_max, t_max_each, out, stream)
                 : launch_occluded_2<THREADS, MODE, false>(S, rays, n, t_min, t_max, t_max_each, out, stream);
}

// rt_scene_occluded: the node / primitive placement the trace kernel uses (`wide`, as launch_features);
// `closest`: the traverse4 instance
hipError_t launch_occluded(const DScene& S, bool wide, bool closest, const double* rays, int n, double t_min,
                           double t_max, const double* t_max_each, uint8_t* out, hipStream_t stream) {
  if (S.exts) return hipErrorInvalidValue;  // (the caller refuses book-2 scenes)
  if (n <= 0) return hipSuccess;
  if (wide) {
    if (S.n_lds_prims > 0)
      return launch_occluded_1<kOccThreadsWide, kSceneLds>(S, closest, rays, n, t_min, t_max, t_max_each, out, stream);
    return launch_occluded_1<kOccThreadsWide, kNodesLds>(S, closest, rays, n, t_min, t_max, t_max_each, out, stream);
  }
  const int mode = S.n_lds_nodes4 >= S.n_nodes4 ? kNodesLds : (S.n_lds_nodes4 == 0 ? kNodesGlobal : kNodesMixed);
  switch (mode) {
    case kNodesLds: return launch_occluded_1<kHitThreads, kNodesLds>(S, closest, rays, n, t_min, t_max, t_max_each, out, stream);
    case kNodesGlobal: return launch_occluded_1<kHitThreads, kNodesGlobal>(S, closest, rays, n, t_min, t_max, t_max_each, out, stream);
    default: return launch_occluded_1<kHitThreads, kNodesMixed>(S, closest, rays, n, t_min, t_max, t_max_each, out, stream);
  }
}

template <int THREADS, int MODE>
static hipError_t launch_ao_1(const DScene& S, const DCamera& C, uint64_t seed, int s_begin, int s_end, int chain,
                              double radius, double* ao, hipStream_t stream) {
  const int tiles_x = (C.width + kTile - 1) / kTile, tiles_y = (C.height + kTile - 1) / kTile;
  const int n_tiles = tiles_x * tiles_y;
  const int per_block = THREADS / kWave;
  const int blocks = (n_tiles + per_block - 1) / per_block;
  const size_t lds = occ_lds_bytes<THREADS, MODE>(S);
  hipError_t e = hipFuncSetAttribute((const void*)ao_kernel<THREADS, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((ao_kernel<THREADS, MODE>), dim3(blocks), dim3(THREADS), lds, stream, S, C, seed, s_begin, s_end,
                     chain, radius, tiles_x, n_tiles, ao);
  return hipGetLastError();
}

// rt_render_ao: block and placement chosen as launch_features does
hipError_t launch_ao(const DScene& S, bool wide, const DCamera& C, uint64_t seed, int s_begin, int s_end, int chain,
                     double radius, double* ao, hipStream_t stream) {
  if (S.exts) return hipErrorInvalidValue;  // (the caller refuses book-2 scenes)
  if (wide) {
    if (S.n_lds_prims > 0) return launch_ao_1<kOccThreadsWide, kSceneLds>(S, C, seed, s_begin, s_end, chain, radius, ao, stream);
    return launch_ao_1<kOccThreadsWide, kNodesLds>(S, C, seed, s_begin, s_end, chain, radius, ao, stream);
  }
  const int mode = S.n_lds_nodes4 >= S.n_nodes4 ? kNodesLds : (S.n_lds_nodes4 == 0 ? kNodesGlobal : kNodesMixed);
  switch (mode) {
    case kNodesLds: return launch_ao_1<kHitThreads, kNodesLds>(S, C, seed, s_begin, s_end, chain, radius, ao, stream);
    case kNodesGlobal: return launch_ao_1<kHitThreads, kNodesGlobal>(S, C, seed, s_begin, s_end, chain, radius, ao, stream);
    default: return launch_ao_1<kHitThreads, kNodesMixed>(S, C, seed, s_begin, s_end, chain, radius, ao, stream);
  }
}

}  // namespace rt
