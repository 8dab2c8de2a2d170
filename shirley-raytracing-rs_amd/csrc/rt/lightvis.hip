// lightvis.hip — the trace kernel of rt_scene_light_visibility (include/shirley_rt.h has the definition,
// operation for operation): K shadow rays from every cell of the light grid to every listed light.
//
// The kernel stands in the frame of pass_frame.h exactly as occluded_kernel does (occlusion.hip): the block's LDS
// layout, the staged nodes, the placements, the any-hit walk occluded4.  One lane per (cell, light, ray), the ray
// in the low bits, so the K lanes of a pair are consecutive lanes of one wave (K divides 64) and the pair's mask
// is a slice of the wave's ballot, written by the group's first lane with a plain store: no atomics, no LDS
// reduction.  Lanes past the end stay for the ballot, contribute 0 and write nothing.
// Only + - * /, sqrt_rn, comparisons and selects in the header's order (the build never fuses a*b+c).
// Reference scenes only (no book-2 records): EXT = false instances.
#include <hip/hip_runtime.h>

#include "direct.h"
#include "lightvis.h"
#include "pass_frame.h"

namespace rt {

template <int THREADS, int MODE>
__global__ __launch_bounds__(THREADS) void lightvis_kernel(DScene S, const DLight* __restrict__ lights, int n_lights,
                                                           DLightGrid G, DLightVisCells Z, uint64_t seed, int log2k,
                                                           uint32_t pairs, uint32_t* __restrict__ masks,
                                                           uint32_t* __restrict__ wave_traced) {
  extern __shared__ unsigned char lds_raw[];
  const BlockLds<DNode4F> L = carve_block_lds<MODE, DNode4F>(S, lds_raw);
  stage_nodes4<MODE>(S, L.nodes, L.prims);
  // (< 2^27 + THREADS: lightvis.h)
  const uint32_t g = blockIdx.x * (uint32_t)THREADS + threadIdx.x;
  const uint32_t pair = g >> log2k;
  const uint32_t i = g & ((1u << log2k) - 1u);
  const bool live = pair < pairs;
  bool bit = false, traced = false;
  if (live) {
    const uint32_t c = pair / (uint32_t)n_lights, j = pair - c * (uint32_t)n_lights;
    const uint32_t nx = (uint32_t)G.n[0], ny = (uint32_t)G.n[1];
    const uint32_t cz = c / (nx * ny), cy = (c - cz * (nx * ny)) / nx, cx = c - (cz * ny + cy) * nx;
    // the cell point: draws 0, 1, 2 of (seed, c, i)
    Rng rng{c, i, 0u, 0u, 0u};
    const double x0 = (G.lo[0] + (double)cx * Z.size[0]) + rng_next(rng, seed) * Z.size[0];
    const double x1 = (G.lo[1] + (double)cy * Z.size[1]) + rng_next(rng, seed) * Z.size[1];
    const double x2 = (G.lo[2] + (double)cz * Z.size[2]) + rng_next(rng, seed) * Z.size[2];
    const v3 x = V(x0, x1, x2);
    const DLight& Q = lights[j];
    bool aim = true;
    v3 y;
    if (Q.geometry == RT_GEOM_SPHERE) {  // the sphere's point nearest to x
      const v3 q = V(Q.p[0], Q.p[1], Q.p[2]);
      const double r = Q.p[3];
      const v3 e = x - q;
      const double e2 = len2(e);
      aim = e2 > r * r;
      const double le = sqrt_rn(e2);
      y = V(q.x + r * (e.x / le), q.y + r * (e.y / le), q.z + r * (e.z / le));
    } else {  // a uniform point of the rect on draws 4 + 2j, 5 + 2j
      Rng rr{c, i, 4u + 2u * j, 0u, 0u};
      y = rect_light_point(Q, Q.geometry, rr, seed);
    }
    const v3 w = y - x;
    traced = aim && len2(w) > 0.0;
    bit = !traced;
    if (traced) {
      unsigned visits = 0, ptests = 0;
      bit = !occluded4<THREADS, MODE>(S, L.nodes, L.prims, x, w, kShadowTMin, kShadowTMax, L.stk, visits, ptests);
    }
  }
  const unsigned long long seen = __ballot(bit);
  const unsigned long long shot = __ballot(traced);
  const uint32_t lane = threadIdx.x % kWave;
  if (live && i == 0u) {
    const unsigned long long field = (1ull << (1u << log2k)) - 1ull;
    masks[pair] = (uint32_t)((seen >> lane) & field);
  }
  if (live && lane == 0u) wave_traced[g / kWave] = (uint32_t)__popcll(shot);
}

hipError_t launch_lightvis(const DScene& S, bool wide, const DLight* lights, int n_lights, const DLightGrid& grid,
                           const DLightVisCells& cells, uint64_t seed, int rays, uint32_t pairs, uint32_t* masks,
                           uint32_t* wave_traced, hipStream_t stream) {
  if (S.exts) return hipErrorInvalidValue;  // (the caller refuses book-2 scenes)
  int log2k = 0;
  while (log2k < 6 && (1 << log2k) != rays) ++log2k;
  if ((1 << log2k) > kLightVisMaxRays || n_lights < 1 || pairs > kLightVisMaxPairs) return hipErrorInvalidValue;
  if (pairs == 0) return hipSuccess;
  const uint32_t lanes = pairs << log2k;
  return dispatch_placement<kPassThreadsWide>(S, wide, [&](auto threads, auto mode) {
    constexpr int T = decltype(threads)::value, M = decltype(mode)::value;
    return launch_block(lightvis_kernel<T, M>, (int)((lanes + (uint32_t)T - 1u) / (uint32_t)T), T,
                        block_lds_bytes<M>(S, node4_bytes(false), T), stream, S, lights, n_lights, grid, cells, seed,
                        log2k, pairs, masks, wave_traced);
  });
}

}  // namespace rt
