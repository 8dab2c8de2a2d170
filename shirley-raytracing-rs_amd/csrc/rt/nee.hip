// nee.hip — rt_render_nee's launch: the uniform instances of nee_kernel (nee_kernel.h), one wave
// per tile of the frame.
#include "nee_kernel.h"

namespace rt {

// rt_render_nee; `grid` (null: the uniform pick) is read only where n_lights > 0; `sample`: kSampleArea, kSampleCone
// or kSampleAll, the instances' sample kind
hipError_t launch_nee(const DScene& S, bool wide, bool mis, const DCamera& C, uint64_t seed, int s_begin, int s_end,
                      int max_depth, const DLight* lights, int n_lights, const DLightGrid* grid, int sample,
                      const int32_t* prim_light, double* accum, hipStream_t stream) {
  if (S.exts) return hipErrorInvalidValue;  // (the caller refuses book-2 scenes)
  if (!accum || !prim_light || (n_lights > 0 && !lights)) return hipErrorInvalidValue;
  if (grid && n_lights > 0 && !grid->cdf) return hipErrorInvalidValue;
  const TileGrid G = tile_grid(C);
  return dispatch_placement<kPassThreadsWide>(S, wide, [&](auto threads, auto mode) {
    constexpr int T = decltype(threads)::value, M = decltype(mode)::value;
    return nee_instance<T, M, false>(mis, grid, n_lights, sample, [&](auto kernel, auto g) {
      return launch_block(kernel, G.blocks(T), T, block_lds_bytes<M>(S, node4_bytes(false), T), stream, S, C, seed,
                          s_begin, s_end, max_depth, G.tiles_x, G.n_tiles, lights, n_lights, prim_light, accum, g,
                          NoNeeAdapt{});
    });
  });
}

}  // namespace rt
