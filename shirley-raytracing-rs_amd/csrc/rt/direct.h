// direct.h — the one-light-sample direct-lighting estimator of rt_render_direct (include/shirley_rt.h has its
// definition, operation for operation), as a device function of its own so that the path
// integrator (nee.hip) calls the same body at every Lambertian / FairyLight vertex.
//
// Only + - * /, sqrt_rn, comparisons and selects in the header's order (the build never fuses a*b+c), on the
// path's own draws; the shadow ray goes through the any-hit walk occluded4 (occlusion.h).
#pragma once

#include "light_pick.h"
#include "occlusion.h"

namespace rt {

constexpr double kDirectPi = 3.141592653589793;
// the shadow ray's interval in units of the vertex-to-sample vector: it stops 2^-20 short of the light
constexpr double kShadowTMin = 0.001;
constexpr double kShadowTMax = 1.0 - 0x1p-20;

// The estimate at a vertex (x, n) with scatter attenuation a, n_lights >= 1.  Consumes the path's draws
// D (the pick), then two (rect) or three per attempt (sphere).  `taken` reports that the vertex took a light
// sample (a cut or occluded one included): the path integrator (nee.hip) then weights the emission its scatter
// lands on.  MIS: the sample carries the balance-heuristic weight against the Lambertian scatter, whose density
// in area measure at the light is gs = ((cx * cy) / d2) / pi, the light sample's being pl = 1 / (area * L):
// g = (1 / pl) * (pl / (pl + gs)) * gs = gs / (pl + gs) in place of gs / pl (rt_render_nee, shirley_rt.h).
// PICK (light_pick.h): kPickGrid takes the light from the vertex's cell of `grid` on the same draw D, with
// probability pk, so pl = pk / area (rt_scene_light_pick); `cell` receives the vertex's cell, which
// the path integrator keeps for the weight of the hit its scatter lands on.  A uniform instance leaves it alone.
template <int THREADS, int MODE, bool MIS, int PICK>
__device__ __forceinline__ v3 direct_light(const DScene& S, const DNode4F* lds_nodes, const DPrim* lds_prims,
                                           const DLight* __restrict__ lights, int n_lights, Rng& rng, uint64_t seed,
                                           v3 x, v3 n, v3 a, unsigned* stk, unsigned& visits, unsigned& ptests,
                                           bool& taken, const typename PickGrid<PICK>::type& grid, int& cell) {
  taken = true;
  const double nl = (double)n_lights;
  int li;
  double pk = 1.0;
  if constexpr (PICK == kPickGrid) {
    cell = light_cell(grid, x.x, x.y, x.z);
    li = light_pick(grid, cell, n_lights, rng_next(rng, seed), pk);
  } else {
    const int pick = (int)(rng_next(rng, seed) * nl);
    li = pick < n_lights - 1 ? pick : n_lights - 1;
  }
  const DLight& L = lights[li];
  const int geom = L.geometry;
  v3 y, u = V(0.0, 0.0, 0.0);
  if (geom == RT_GEOM_SPHERE) {
    u = unit(random_in_unit_sphere(rng, seed));
    y = V(L.p[0], L.p[1], L.p[2]) + scale(u, L.p[3]);
  } else {
    const double xi1 = rng_next(rng, seed);
    const double xi2 = rng_next(rng, seed);
    const double c1 = L.p[0] + xi1 * (L.p[1] - L.p[0]);
    const double c2 = L.p[2] + xi2 * (L.p[3] - L.p[2]);
    const double off = L.p[4];
    // (d1, d2, axis): RECT_XY (x, y, z), RECT_YZ (y, z, x), RECT_XZ (x, z, y) — geometry/rect.rs
    y = geom == RT_GEOM_RECT_XY ? V(c1, c2, off) : geom == RT_GEOM_RECT_YZ ? V(off, c1, c2) : V(c1, off, c2);
  }
  const v3 w = y - x;
  const double d2 = len2(w);
  const double dist = sqrt_rn(d2);
  const double cx = dot(n, w) / dist;
  double cy;
  if (geom == RT_GEOM_SPHERE) {
    cy = -dot(u, w) / dist;
  } else {
    const double wa = geom == RT_GEOM_RECT_XY ? w.z : geom == RT_GEOM_RECT_YZ ? w.x : w.y;
    cy = fabs(wa) / dist;
  }
  if (!(cx > 0.0 && cy > 0.0)) return V(0.0, 0.0, 0.0);  // back faces, and a NaN
  if (occluded4<THREADS, MODE>(S, lds_nodes, lds_prims, x, w, kShadowTMin, kShadowTMax, stk, visits, ptests))
    return V(0.0, 0.0, 0.0);
  v3 le = V(L.color[0], L.color[1], L.color[2]);
  if (L.emitter == RT_MAT_FAIRY_LIGHT) le = scale(le, cy);  // lighting.rs:59-65 for the ray (x, w)
  double g;
  if (MIS) {
    const double gs = ((cx * cy) / d2) / kDirectPi;
    const double pl = PICK == kPickGrid ? pk / L.area : 1.0 / (L.area * nl);
    g = gs / (pl + gs);
  } else {
    g = ((cx * cy) / d2) * ((PICK == kPickGrid ? L.area / pk : L.area * nl) / kDirectPi);
  }
  return scale(hmul(a, le), g);
}

// The plain form (rt_render_direct's estimator).
template <int THREADS, int MODE, int PICK>
__device__ __forceinline__ v3 direct_light(const DScene& S, const DNode4F* lds_nodes, const DPrim* lds_prims,
                                           const DLight* __restrict__ lights, int n_lights, Rng& rng, uint64_t seed,
                                           v3 x, v3 n, v3 a, unsigned* stk, unsigned& visits, unsigned& ptests,
                                           const typename PickGrid<PICK>::type& grid) {
  bool taken;
  int cell;
  return direct_light<THREADS, MODE, false, PICK>(S, lds_nodes, lds_prims, lights, n_lights, rng, seed, x, n, a, stk,
                                                  visits, ptests, taken, grid, cell);
}

}  // namespace rt
