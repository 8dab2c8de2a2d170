// occlusion.hip — rt_scene_occluded and rt_render_ao (include/shirley_rt.h, ABI 11).
//
// Both kernels stand in the frame of pass_frame.h (the block's LDS layout, the placements, the launch).
// occluded_kernel: one ray per lane, answering through the any-hit walk occluded4 (occlusion.h) or, in its second
// instance (CLOSEST), through traverse4 (`best >= 0`); both give the same bytes.
// ao_kernel: a tile pass — one wave per 8x8 tile, one lane per pixel, the sample loop inside the lane, the camera
// ray and the dielectric chain to the feature vertex — without a texture, so without the wave-wide marble: lanes
// outside the image leave after the staging.  At the feature vertex it forms the renderer's Lambertian scatter
// direction on the path's own draws and asks occluded4 along it.
// Reference scenes only (no book-2 records): EXT = false instances.
#include <hip/hip_runtime.h>

#include "occlusion.h"
#include "pass_frame.h"
#include "rt_launch.h"

namespace rt {

template <int THREADS, int MODE, bool CLOSEST>
__global__ __launch_bounds__(THREADS) void occluded_kernel(DScene S, const double* __restrict__ rays, int n,
                                                           double t_min, double t_max,
                                                           const double* __restrict__ t_max_each,
                                                           uint8_t* __restrict__ out) {
  extern __shared__ unsigned char lds_raw[];
  const BlockLds<DNode4F> L = carve_block_lds<MODE, DNode4F>(S, lds_raw);
  stage_nodes4<MODE>(S, L.nodes, L.prims);
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
    occ = traverse4<THREADS, MODE, false>(S, L.nodes, L.prims, o, d, t_min, t_best, face, L.stk, rk, 0ull, visits,
                                          ptests RT_STAT_ARG(steps)) >= 0;
  } else {
    occ = occluded4<THREADS, MODE>(S, L.nodes, L.prims, o, d, t_min, tm, L.stk, visits, ptests);
  }
  out[i] = occ ? 1 : 0;
}

template <int THREADS, int MODE>
__global__ __launch_bounds__(THREADS) void ao_kernel(DScene S, DCamera C, uint64_t seed, int s_begin, int s_end,
                                                     int chain, double radius, int tiles_x, int n_tiles,
                                                     double* __restrict__ ao) {
  extern __shared__ unsigned char lds_raw[];
  const BlockLds<DNode4F> L = carve_block_lds<MODE, DNode4F>(S, lds_raw);
  stage_nodes4<MODE>(S, L.nodes, L.prims);
  const TileLane T = tile_lane<THREADS>(tiles_x);
  if (T.tile >= n_tiles || !T.active(C)) return;  // (nothing wave-wide follows)
  const int px = T.px, py = T.py;
  const uint32_t pix = T.pix(C);
  double sum = 0.0;
  unsigned visits = 0, ptests = 0;
#ifdef RT_PHASE_TIMING
  unsigned long long steps = 0;
#endif
  for (int s = s_begin; s < s_end; ++s) {
    Rng rng{pix, (uint32_t)s, 0u, 0u, 0u};
    v3 o, d;
    sample_ray(C, rng, seed, px, py, o, d);
    Hit h;
    bool hit;
    int left = chain;
    for (;;) {  // through at most `chain` dielectric vertices; each kernel keeps this loop
      double t_best = __builtin_inf();
      int face = -1;
      const int prim = traverse4<THREADS, MODE, false>(S, L.nodes, L.prims, o, d, 0.001, t_best, face, L.stk, rng,
                                                       seed, visits, ptests RT_STAT_ARG(steps));
      hit = prim >= 0;
      if (!hit) break;
      const DPrim pr = (MODE == kSceneLds) ? L.prims[prim] : S.prims[prim];
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
    sum += occluded4<THREADS, MODE>(S, L.nodes, L.prims, h.point, w, 0.001, t_max, L.stk, visits, ptests) ? 0.0 : 1.0;
  }
  ao[(size_t)py * (size_t)C.width + (size_t)px] = sum;
}

// rt_scene_occluded; `closest`: the traverse4 instance
hipError_t launch_occluded(const DScene& S, bool wide, bool closest, const double* rays, int n, double t_min,
                           double t_max, const double* t_max_each, uint8_t* out, hipStream_t stream) {
  if (S.exts) return hipErrorInvalidValue;  // (the caller refuses book-2 scenes)
  if (n <= 0) return hipSuccess;
  return dispatch_placement<kPassThreadsWide>(S, wide, [&](auto threads, auto mode) {
    constexpr int T = decltype(threads)::value, M = decltype(mode)::value;
    auto go = [&](auto kernel) {
      return launch_block(kernel, (n + T - 1) / T, T, block_lds_bytes<M>(S, node4_bytes(false), T), stream, S, rays, n,
                          t_min, t_max, t_max_each, out);
    };
    return closest ? go(occluded_kernel<T, M, true>) : go(occluded_kernel<T, M, false>);
  });
}

// rt_render_ao
hipError_t launch_ao(const DScene& S, bool wide, const DCamera& C, uint64_t seed, int s_begin, int s_end, int chain,
                     double radius, double* ao, hipStream_t stream) {
  if (S.exts) return hipErrorInvalidValue;  // (the caller refuses book-2 scenes)
  const TileGrid G = tile_grid(C);
  return dispatch_placement<kPassThreadsWide>(S, wide, [&](auto threads, auto mode) {
    constexpr int T = decltype(threads)::value, M = decltype(mode)::value;
    return launch_block(ao_kernel<T, M>, G.blocks(T), T, block_lds_bytes<M>(S, node4_bytes(false), T), stream, S, C,
                        seed, s_begin, s_end, chain, radius, G.tiles_x, G.n_tiles, ao);
  });
}

}  // namespace rt
