// light_pick.h — the spatially weighted light pick of rt_scene_light_pick (include/shirley_rt.h has its
// definition, operation for operation): the light grid as a kernel argument of its own, the cell of
// a vertex, the one-draw pick from the cell's running sums, and the probability of a light in a cell.
//
// The table is built on the host (scene_compile.cpp build_light_grid).  Only + - * /, comparisons and selects in
// the header's order here too; the search's trip count depends on the light count alone, so it is wave-uniform.
#pragma once

#include <stdint.h>

namespace rt {

// The pick kind: a template parameter of direct_light, direct_kernel and nee_kernel.
constexpr int kPickUniform = 0;  // k = min((int)(xi0 * L), L - 1)
constexpr int kPickGrid = 1;     // from the vertex's cell of the light grid

// The grid as the kernels read it: row c of `cdf` (n_lights binary64 running sums, the last exactly 1.0) is cell
// c = (iz * n[1] + iy) * n[0] + ix.  inv[a] = n[a] / (hi[a] - lo[a]), and 0 where n[a] == 1.
struct DLightGrid {
  const double* cdf;
  double lo[3];
  double inv[3];
  int32_t n[3];
  int32_t pad;
};
// What a uniform instance takes in the grid's place (nothing).
struct NoLightGrid {};
template <int PICK>
struct PickGrid {
  typedef NoLightGrid type;
};
template <>
struct PickGrid<kPickGrid> {
  typedef DLightGrid type;
};

#ifdef __HIPCC__
// One axis of the cell: 0 below the box and for a NaN, n - 1 above it.
__device__ __forceinline__ int light_cell_axis(double x, double lo, double inv, int n) {
  const double q = (x - lo) * inv;
  return !(q >= 0.0) ? 0 : q >= (double)n ? n - 1 : (int)q;
}

__device__ __forceinline__ int light_cell(const DLightGrid& G, double x, double y, double z) {
  const int ix = light_cell_axis(x, G.lo[0], G.inv[0], G.n[0]);
  const int iy = light_cell_axis(y, G.lo[1], G.inv[1], G.n[1]);
  const int iz = light_cell_axis(z, G.lo[2], G.inv[2], G.n[2]);
  return (iz * G.n[1] + iy) * G.n[0] + ix;
}

// p_j(cell) = cdf[j] - cdf[j - 1]: up to rounding, the probability with which light_pick returns j there.
__device__ __forceinline__ double light_prob(const DLightGrid& G, int cell, int n_lights, int j) {
  const double* row = G.cdf + (size_t)cell * (size_t)n_lights;
  return row[j] - (j ? row[j - 1] : 0.0);
}

// The smallest k with xi < cdf[k] in the cell's row (n_lights - 1 when there is none: xi >= 1 or a NaN), by a
// lower-bound search whose range shrinks by the same amounts whatever the comparisons say.
__device__ __forceinline__ int light_pick(const DLightGrid& G, int cell, int n_lights, double xi, double& prob) {
  const double* row = G.cdf + (size_t)cell * (size_t)n_lights;
  int base = 0;
  for (int n = n_lights; n > 1;) {  // the answer is in [base, base + n)
    const int half = n >> 1;
    base = xi < row[base + half - 1] ? base : base + half;
    n -= half;
  }
  prob = row[base] - (base ? row[base - 1] : 0.0);
  return base;
}
#endif

}  // namespace rt
