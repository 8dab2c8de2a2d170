// pass_frame.h — the frame that the tile passes (features.hip, occlusion.hip's ao_kernel, direct.hip, nee.hip)
// and the ray-batch kernels (occlusion.hip's occluded_kernel, trace.hip's hit4_kernel / probe_kernel) stand in
// (DESIGN.md §17): the block's LDS layout, the wave -> tile / lane -> pixel mapping, the launch with its
// placement choice, and steps of a sample's path (its camera ray, a vertex's texture leaf, the wave's marble).
// Plain inline functions; a kernel calls the pieces it needs and keeps what is its own: its list of material
// kinds, its early exits, and its loop through the dielectric chain (DESIGN.md §17 says why).
#pragma once

#include <type_traits>

#include "rt_device.h"

namespace rt {

// Block of the scene-in-LDS placements (`wide`) of the tile passes and of occluded_kernel: the megakernel's
// 1024 threads, which the placement plan sized the LDS stacks for — 16 tiles share one staged copy of the
// scene.  Measured for features_kernel at 16 spp, chain 8 (profiles/denoise/features_block_ab.json): headline
// 1200x800 3.44 ms against 4.49 ms (512 threads) and 6.88 ms (256); Cornell 600x600 0.295 ms against
// 0.268 / 0.231 ms.
constexpr int kPassThreadsWide = kTraceThreadsWide;

// ------------------------------------------------------------------------------------------
// block layout: what stage_nodes4<MODE> copies into the dynamic LDS, then the traversal stacks
// ------------------------------------------------------------------------------------------
// Byte offset of the stacks (trace_lds_bytes, rt_layout.h, without them): the host sizes the block by it and
// the kernel carves by it.
template <int MODE>
__host__ __device__ constexpr size_t stack_offset(const DScene& S, int node4_size) {
  constexpr bool all = MODE == kSceneLds;
  return trace_lds_bytes(S.n_lds_nodes4, node4_size, all ? S.n_lds_prims : 0, all ? S.n_lds_perlin : 0, 0, 0,
                         all ? S.n_lds_mats : 0, all ? S.n_lds_texs : 0);
}
template <int MODE>
inline size_t block_lds_bytes(const DScene& S, int node4_size, int threads) {
  return stack_offset<MODE>(S, node4_size) + trace_lds_bytes(0, 0, 0, 0, S.stack_depth4, threads, 0, 0);
}

template <class N4>
struct BlockLds {
  N4* nodes;
  DPrim* prims;
  const DPerlin* perlin;  // the LDS copy of the Perlin tables, or null (read them from S.perlin)
  unsigned* stk;          // the lane's traversal stack
};
template <int MODE, class N4>
__device__ __forceinline__ BlockLds<N4> carve_block_lds(const DScene& S, unsigned char* lds_raw) {
  BlockLds<N4> L;
  L.nodes = reinterpret_cast<N4*>(lds_raw);
  // (the primitives follow the nodes, at the stack offset of a nodes-only block; the stacks are addressed from
  // them, not from lds_raw: the spelling decides some instances' SGPR spills)
  constexpr int n4 = (int)sizeof(N4);
  L.prims = reinterpret_cast<DPrim*>(lds_raw + stack_offset<kNodesLds>(S, n4));
  L.perlin = (MODE == kSceneLds && S.n_lds_perlin > 0) ? reinterpret_cast<const DPerlin*>(L.prims + S.n_lds_prims)
                                                       : nullptr;
  L.stk = reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(L.prims) +
                                     (stack_offset<MODE>(S, n4) - stack_offset<kNodesLds>(S, n4))) +
          threadIdx.x;
  return L;
}

// ------------------------------------------------------------------------------------------
// tile mapping: one wave per 8x8 tile, one lane per pixel
// ------------------------------------------------------------------------------------------
struct TileGrid {
  int tiles_x, n_tiles;
  int blocks(int threads) const { return (n_tiles + threads / kWave - 1) / (threads / kWave); }
};
inline TileGrid tile_grid(const DCamera& C) {
  const int tiles_x = (C.width + kTile - 1) / kTile, tiles_y = (C.height + kTile - 1) / kTile;
  return TileGrid{tiles_x, tiles_x * tiles_y};
}

// Wave w of the block renders tile blockIdx * (THREADS / 64) + w; lane l its pixel (l % 8, l / 8).  A whole
// wave with tile >= n_tiles leaves together; lanes of an edge tile outside the image are not active(C): a
// kernel with a wave-wide step keeps them, idle, for it.  (active and pix are taken after that exit, not
// before it: the order decides some instances' SGPR spills)
struct TileLane {
  int tile, px, py;
  __device__ bool active(const DCamera& C) const { return px < C.width && py < C.height; }
  // the pixel's path key
  __device__ uint32_t pix(const DCamera& C) const { return (uint32_t)py * (uint32_t)C.width + (uint32_t)px; }
};
template <int THREADS>
__device__ __forceinline__ TileLane tile_lane(int tiles_x) {
  const int tid = threadIdx.x;
  const int lane = tid % kWave;
  TileLane T;
  T.tile = blockIdx.x * (THREADS / kWave) + tid / kWave;
  T.px = (T.tile % tiles_x) * kTile + lane % kTile;
  T.py = (T.tile / tiles_x) * kTile + lane / kTile;
  return T;
}

// ------------------------------------------------------------------------------------------
// launch
// ------------------------------------------------------------------------------------------
inline int node_mode4(const DScene& S) {
  return S.n_lds_nodes4 >= S.n_nodes4 ? kNodesLds : (S.n_lds_nodes4 == 0 ? kNodesGlobal : kNodesMixed);
}

// Allow the dynamic LDS beyond the 64 KiB default (gfx950 has 160 KiB per CU), launch, report.
template <class K, class... A>
hipError_t launch_block(K kernel, int blocks, int threads, size_t lds, hipStream_t stream, A... args) {
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, stream, args...);
  return hipGetLastError();
}

// The node / primitive placement the trace kernel uses: with `wide` the scene-in-LDS block of WIDE_THREADS
// (nodes, and the primitives when the plan placed them), else a kHitThreads block on the placement of the
// 4-wide nodes.  f(threads, mode) takes both as std::integral_constant.
template <int WIDE_THREADS, class F>
hipError_t dispatch_placement(const DScene& S, bool wide, F f) {
  using Wide = std::integral_constant<int, WIDE_THREADS>;
  using Narrow = std::integral_constant<int, kHitThreads>;
  if (wide) {
    if (S.n_lds_prims > 0) return f(Wide{}, std::integral_constant<int, kSceneLds>{});
    return f(Wide{}, std::integral_constant<int, kNodesLds>{});
  }
  switch (node_mode4(S)) {
    case kNodesLds: return f(Narrow{}, std::integral_constant<int, kNodesLds>{});
    case kNodesGlobal: return f(Narrow{}, std::integral_constant<int, kNodesGlobal>{});
    default: return f(Narrow{}, std::integral_constant<int, kNodesMixed>{});
  }
}

// ------------------------------------------------------------------------------------------
// steps of a sample's path
// ------------------------------------------------------------------------------------------
// The camera ray of (pixel, sample): draws 0, 1 (jitter, render.rs:60-63) and the lens-disk draws.
__device__ __forceinline__ void sample_ray(const DCamera& C, Rng& rng, uint64_t seed, int px, int py, v3& o, v3& d) {
  const double jx = (double)px + rng_next(rng, seed);
  const double jy = (double)py + rng_next(rng, seed);
  camera_ray(C, rng, seed, jx, jy, o, d);
}

// Resolve a material's texture to its leaf at p and note whether the leaf needs the wave's marble.
__device__ __forceinline__ int texture_leaf(const DScene& S, int tex, v3 p, bool& need_pn, int& ptab, double& psc) {
  const int leaf = resolve_texture(S, tex, p);
  const DTex& tx = S.texs[leaf];
  if (tx.kind == RT_TEX_PERLIN) {
    need_pn = true;
    ptab = tx.table;
    psc = tx.scale;
  }
  return leaf;
}

// The wave's marble values from the block's Perlin tables (wave-wide: every lane of the wave calls it).
__device__ __forceinline__ double wave_marble(const DScene& S, const DPerlin* lds_perlin, bool need_pn, int ptab,
                                              double psc, v3 p) {
  return lds_perlin ? marble_coop((LdsPerlin*)lds_perlin, need_pn, ptab, psc, p)
                    : marble_coop(S.perlin, need_pn, ptab, psc, p);
}

}  // namespace rt
