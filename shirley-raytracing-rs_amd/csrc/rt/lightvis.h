// lightvis.h — the launch wrapper of lightvis.hip (rt_scene_light_visibility; include/shirley_rt.h has the
// definition, operation for operation), and what the kernel takes besides the light grid.
#pragma once

#include <hip/hip_runtime.h>

#include "light_pick.h"
#include "rt_layout.h"

namespace rt {

// size_a = (hi_a - lo_a) / (double)n_a of the grid (scene_compile.cpp build_light_grid computes the same
// quotient), from which a cell's corner is lo_a + (double)i_a * size_a.
struct DLightVisCells {
  double size[3];
};

// Lanes of a launch: pairs * rays, one per (cell, light, ray) with the ray in the low bits.  The table limit
// (kLightGridMaxEntries = 2^22 pairs) and rays <= 32 bound it by 2^27, and a launch rounds it up by less than
// one block, so 32-bit lane, pair and cell numbers suffice; launch_lightvis refuses anything beyond.
constexpr uint32_t kLightVisMaxPairs = 1u << 22;
constexpr int kLightVisMaxRays = 32;

// masks [pairs]: bit i of masks[c * n_lights + j] is ray i's.  wave_traced [ceil(pairs * rays / 64)]: the rays
// each wave traced (bits decided without a ray are not counted).  `rays` is 1, 2, 4, 8, 16 or 32.
hipError_t launch_lightvis(const DScene& S, bool wide, const DLight* lights, int n_lights, const DLightGrid& grid,
                           const DLightVisCells& cells, uint64_t seed, int rays, uint32_t pairs, uint32_t* masks,
                           uint32_t* wave_traced, hipStream_t stream);

}  // namespace rt
