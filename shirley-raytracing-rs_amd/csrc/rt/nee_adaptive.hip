// nee_adaptive.hip — rt_render_nee_adaptive's launch: the ADAPT instances of nee_kernel (nee_kernel.h; DESIGN.md
// §22) in a file of their own, so that they compile beside nee.hip's.  One launch renders the whole adaptive
// frame: the grid is what the device holds at once (never more blocks than the tiles need), and its waves take
// the tiles from the counter.
#include <algorithm>

#include "nee_kernel.h"

namespace rt {

// `ad.counter` must have been cleared on `stream`; max_blocks > 0 sets the grid in place of the device's fill
// (SHIRLEY_NEE_BLOCKS: below the fill or above it, where blocks queue for a CU — no wave waits for another, so
// residency is no condition — but never more blocks than the tiles need; the frame is the same for every grid).
// The other arguments are launch_nee's, over the sample range [0, samples).
hipError_t launch_nee_adaptive(const DScene& S, bool wide, bool mis, const DCamera& C, uint64_t seed, int samples,
                               int max_depth, const DLight* lights, int n_lights, const DLightGrid* grid, int sample,
                               const int32_t* prim_light, double* accum, const NeeAdapt& ad, int cu_count,
                               int max_blocks, hipStream_t stream) {
  if (S.exts) return hipErrorInvalidValue;  // (the caller refuses book-2 scenes)
  if (!accum || !prim_light || (n_lights > 0 && !lights)) return hipErrorInvalidValue;
  if (grid && n_lights > 0 && !grid->cdf) return hipErrorInvalidValue;
  if (!ad.counter || !ad.moments || !ad.counts || ad.batch < 1 || ad.min_samples < 2 * ad.batch ||
      ad.step < ad.batch || samples < ad.min_samples || max_depth < 1)
    return hipErrorInvalidValue;
  const TileGrid G = tile_grid(C);
  return dispatch_placement<kPassThreadsWide>(S, wide, [&](auto threads, auto mode) {
    constexpr int T = decltype(threads)::value, M = decltype(mode)::value;
    return nee_instance<T, M, true>(mis, grid, n_lights, sample, [&](auto kernel, auto g) {
      const size_t lds = block_lds_bytes<M>(S, node4_bytes(false), T);
      hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      int per_cu = 0;
      e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, T, lds);
      if (e != hipSuccess) return e;
      const int fill = std::max(1, cu_count) * std::max(1, per_cu);
      const int blocks = std::min(G.blocks(T), max_blocks > 0 ? max_blocks : fill);
      return launch_block(kernel, blocks, T, lds, stream, S, C, seed, 0, samples, max_depth, G.tiles_x, G.n_tiles,
                          lights, n_lights, prim_light, accum, g, ad);
    });
  });
}

}  // namespace rt
