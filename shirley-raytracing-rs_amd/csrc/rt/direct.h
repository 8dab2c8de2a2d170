// direct.h — the one-light-sample direct-lighting estimator of rt_render_direct (include/shirley_rt.h has its
// definition, operation for operation), as a device function of its own so that the path
// integrator (nee.hip) calls the same body at every Lambertian / FairyLight vertex.
//
// Only + - * /, sqrt_rn, comparisons and selects in the header's order (the build never fuses a*b+c; a
// kSampleAll instance also calls pl_sin, pl_cos and pl_acos, which are such operations: light_rect.h), on the
// path's own draws; the shadow ray goes through the any-hit walk occluded4 (occlusion.h).  The sample itself
// (light_sample_point: the pick, the point on the light, w, the cosines, the cut) and its value's factor
// (light_sample_g) are functions of their own, which the probe kernel of rt_light_sample_at (direct.hip) runs
// without the shadow ray.
#pragma once

#include "light_pick.h"
#include "occlusion.h"
#define RT_CONE_SQRT sqrt_rn  // (the kernels' correctly rounded sqrt)
#include "light_cone.h"
#include "light_rect.h"

namespace rt {

constexpr double kDirectPi = 3.141592653589793;
// the shadow ray's interval in units of the vertex-to-sample vector: it stops 2^-20 short of the light
constexpr double kShadowTMin = 0.001;
constexpr double kShadowTMax = 1.0 - 0x1p-20;

// A light sample before its shadow ray: the light, why it contributes nothing without one (flags), the vector
// from the vertex to the sample, the two cosines and what the value's factor needs besides.
constexpr int kLightCut = 1;       // !(cx > 0 && cy > 0)
constexpr int kLightInside = 2;    // kSampleCone: the vertex is inside or on the sphere, !(dc2 > r*r)
constexpr int kLightCoplanar = 4;  // kSampleAll: the vertex lies in the rect's plane, z0 == 0
constexpr int kLightSmall = 8;     // kSampleAll: !(S >= 2^-20), the rect's sample is the area form's (not zeroed)
constexpr int kLightZero = kLightCut | kLightInside | kLightCoplanar;  // the sample contributes nothing
struct LightSample {
  int li, flags;
  v3 w;
  double cx, cy, d2;
  double pk;  // the pick's probability (kPickGrid)
  double om;  // 1 - cos(theta_max) of the cone (a sphere light by solid angle); S of a rect's (kSampleAll)
};

// A uniform point of a rect light on the path's next two draws.
__device__ __forceinline__ v3 rect_light_point(const DLight& L, int geom, Rng& rng, uint64_t seed) {
  const double xi1 = rng_next(rng, seed);
  const double xi2 = rng_next(rng, seed);
  const double c1 = L.p[0] + xi1 * (L.p[1] - L.p[0]);
  const double c2 = L.p[2] + xi2 * (L.p[3] - L.p[2]);
  const double off = L.p[4];
  // (d1, d2, axis): RECT_XY (x, y, z), RECT_YZ (y, z, x), RECT_XZ (x, z, y) — geometry/rect.rs
  return geom == RT_GEOM_RECT_XY ? V(c1, c2, off) : geom == RT_GEOM_RECT_YZ ? V(off, c1, c2) : V(c1, off, c2);
}

// The sample at a vertex (x, n), n_lights >= 1.  Consumes the path's draws D (the pick), then two (rect), three
// per attempt (sphere, kSampleArea) or two per attempt (sphere, kSampleCone: the lens's disk; none from inside).
// PICK (light_pick.h): kPickGrid takes the light from the vertex's cell of `grid` on the same draw D, with
// probability pk (rt_scene_light_pick); `cell` receives the vertex's cell.  A uniform instance
// leaves it alone.  SAMPLE (light_cone.h): kSampleCone draws a sphere light's sample from the cone it subtends
// (rt_scene_light_sampling) and samples rects by area; kSampleAll (light_rect.h)
// samples spheres as kSampleCone does and rects by the spherical rectangle they subtend, on the area form's two draws.
template <int PICK, int SAMPLE>
__device__ __forceinline__ LightSample light_sample_point(const DLight* __restrict__ lights, int n_lights, Rng& rng,
                                                          uint64_t seed, v3 x, v3 n,
                                                          const typename PickGrid<PICK>::type& grid, int& cell) {
  LightSample s;
  const double nl = (double)n_lights;
  s.pk = 1.0;
  s.om = 0.0;
  if constexpr (PICK == kPickGrid) {
    cell = light_cell(grid, x.x, x.y, x.z);
    s.li = light_pick(grid, cell, n_lights, rng_next(rng, seed), s.pk);
  } else {
    const int pick = (int)(rng_next(rng, seed) * nl);
    s.li = pick < n_lights - 1 ? pick : n_lights - 1;
  }
  const DLight& L = lights[s.li];
  const int geom = L.geometry;
  if constexpr (SAMPLE != kSampleArea) {
    // every branch leaves w and cy's numerator: with the area form's y and u below, set in one branch and read
    // after both, these instances kept the two vectors in scratch
    v3 w;
    double cyn;
    if (geom == RT_GEOM_SPHERE) {
      const c3 c{L.p[0], L.p[1], L.p[2]}, xv{x.x, x.y, x.z};
      c3 wc, cw, cu;
      double dc2;
      if (!cone_open(c, L.p[3], xv, wc, dc2, s.om)) {
        s.flags = kLightInside;
        s.w = V(0.0, 0.0, 0.0);
        s.cx = s.cy = s.d2 = 0.0;
        return s;
      }
      const v3 pd = random_in_unit_disk(rng, seed);
      cone_sample(c, L.p[3], xv, wc, dc2, s.om, pd.x, pd.y, cw, cu);
      w = V(cw.x, cw.y, cw.z);
      cyn = -dot(V(cu.x, cu.y, cu.z), w);
    } else if constexpr (SAMPLE == kSampleAll) {
      // (d1, d2, axis) as in rect_light_point; the view's frame is that permutation of the coordinates
      const double xd1 = geom == RT_GEOM_RECT_YZ ? x.y : x.x;
      const double xd2 = geom == RT_GEOM_RECT_XY ? x.y : x.z;
      const double xa = geom == RT_GEOM_RECT_XY ? x.z : geom == RT_GEOM_RECT_YZ ? x.x : x.y;
      RectView rv;
      const int open = rect_open(L.p, xd1, xd2, xa, rv);
      if (open == kRectCoplanar) {
        s.flags = kLightCoplanar;
        s.w = V(0.0, 0.0, 0.0);
        s.cx = s.cy = s.d2 = 0.0;
        return s;
      }
      const double xi1 = rng_next(rng, seed);
      const double xi2 = rng_next(rng, seed);
      double w1, w2, wa;
      if (open == kRectOpen) {
        s.om = rv.S;
        rect_sample(rv, xi1, xi2, w1, w2, wa);
      } else {  // the area form's point on the same two draws
        w1 = (L.p[0] + xi1 * (L.p[1] - L.p[0])) - xd1;
        w2 = (L.p[2] + xi2 * (L.p[3] - L.p[2])) - xd2;
        wa = L.p[4] - xa;
      }
      w = geom == RT_GEOM_RECT_XY ? V(w1, w2, wa) : geom == RT_GEOM_RECT_YZ ? V(wa, w1, w2) : V(w1, wa, w2);
      cyn = fabs(wa);
      s.w = w;
      s.d2 = len2(w);
      const double dist = sqrt_rn(s.d2);
      s.cx = dot(n, w) / dist;
      s.cy = cyn / dist;
      s.flags = (!(s.cx > 0.0 && s.cy > 0.0) ? kLightCut : 0) | (open == kRectOpen ? 0 : kLightSmall);
      return s;
    } else {
      w = rect_light_point(L, geom, rng, seed) - x;
      cyn = fabs(geom == RT_GEOM_RECT_XY ? w.z : geom == RT_GEOM_RECT_YZ ? w.x : w.y);
    }
    s.w = w;
    s.d2 = len2(w);
    const double dist = sqrt_rn(s.d2);
    s.cx = dot(n, w) / dist;
    s.cy = cyn / dist;
  } else {
    v3 y, u = V(0.0, 0.0, 0.0);
    if (geom == RT_GEOM_SPHERE) {
      u = unit(random_in_unit_sphere(rng, seed));
      y = V(L.p[0], L.p[1], L.p[2]) + scale(u, L.p[3]);
    } else {
      y = rect_light_point(L, geom, rng, seed);
    }
    const v3 w = y - x;
    s.w = w;
    s.d2 = len2(w);
    const double dist = sqrt_rn(s.d2);
    s.cx = dot(n, w) / dist;
    if (geom == RT_GEOM_SPHERE) {
      s.cy = -dot(u, w) / dist;
    } else {  // (the reference's emitters radiate from both faces)
      const double wa = geom == RT_GEOM_RECT_XY ? w.z : geom == RT_GEOM_RECT_YZ ? w.x : w.y;
      s.cy = fabs(wa) / dist;
    }
  }
  s.flags = !(s.cx > 0.0 && s.cy > 0.0) ? kLightCut : 0;  // back faces, and a NaN
  return s;
}

// The factor g of an uncut sample's value (a * Le) * g.  MIS: the sample carries the balance-heuristic weight
// against the Lambertian scatter, whose density in area measure at the light is gs = ((cx * cy) / d2) / pi, the
// light sample's being pl = 1 / (area * L), or pk / area under the grid pick:
// g = (1 / pl) * (pl / (pl + gs)) * gs = gs / (pl + gs) in place of gs / pl (rt_render_nee, shirley_rt.h).
// A cone sample's densities are per solid angle: gs = cx / pi, pl = 1 / (2 pi om L) or pk / (2 pi om); so are a
// spherical rectangle's (kSampleAll, a rect whose sample is not the area form's): pl = 1 / (S L) or pk / S.
template <bool MIS, int PICK, int SAMPLE>
__device__ __forceinline__ double light_sample_g(const DLight& L, const LightSample& s, double nl) {
  if (SAMPLE == kSampleAll && L.geometry != RT_GEOM_SPHERE && !(s.flags & kLightSmall)) {
    if (MIS) {
      const double gs = s.cx / kDirectPi;
      const double pl = PICK == kPickGrid ? s.pk / s.om : 1.0 / (s.om * nl);
      return gs / (pl + gs);
    }
    return s.cx * ((PICK == kPickGrid ? s.om / s.pk : s.om * nl) / kDirectPi);
  }
  if (SAMPLE != kSampleArea && L.geometry == RT_GEOM_SPHERE) {
    if (MIS) {
      const double gs = s.cx / kDirectPi;
      const double pl = PICK == kPickGrid ? s.pk / ((2.0 * kDirectPi) * s.om)
                                          : 1.0 / (((2.0 * kDirectPi) * s.om) * nl);
      return gs / (pl + gs);
    }
    return s.cx * (PICK == kPickGrid ? (2.0 * s.om) / s.pk : (2.0 * s.om) * nl);
  }
  if (MIS) {
    const double gs = ((s.cx * s.cy) / s.d2) / kDirectPi;
    const double pl = PICK == kPickGrid ? s.pk / L.area : 1.0 / (L.area * nl);
    return gs / (pl + gs);
  }
  return ((s.cx * s.cy) / s.d2) * ((PICK == kPickGrid ? L.area / s.pk : L.area * nl) / kDirectPi);
}

// The estimate at a vertex (x, n) with scatter attenuation a, n_lights >= 1: light_sample_point, the shadow ray,
// the value.  `taken` reports that the vertex took a light sample (a cut, inside, coplanar or occluded one included): the
// path integrator (nee.hip) then weights the emission its scatter lands on, and keeps `cell` (kPickGrid) for it.
template <int THREADS, int MODE, bool MIS, int PICK, int SAMPLE>
__device__ __forceinline__ v3 direct_light(const DScene& S, const DNode4F* lds_nodes, const DPrim* lds_prims,
                                           const DLight* __restrict__ lights, int n_lights, Rng& rng, uint64_t seed,
                                           v3 x, v3 n, v3 a, unsigned* stk, unsigned& visits, unsigned& ptests,
                                           bool& taken, const typename PickGrid<PICK>::type& grid, int& cell) {
  taken = true;
  const LightSample s = light_sample_point<PICK, SAMPLE>(lights, n_lights, rng, seed, x, n, grid, cell);
  if (SAMPLE == kSampleAll ? (s.flags & kLightZero) != 0 : s.flags != 0) return V(0.0, 0.0, 0.0);
  if (occluded4<THREADS, MODE>(S, lds_nodes, lds_prims, x, s.w, kShadowTMin, kShadowTMax, stk, visits, ptests))
    return V(0.0, 0.0, 0.0);
  const DLight& L = lights[s.li];
  v3 le = V(L.color[0], L.color[1], L.color[2]);
  if (L.emitter == RT_MAT_FAIRY_LIGHT) le = scale(le, s.cy);  // lighting.rs:59-65 for the ray (x, w)
  return scale(hmul(a, le), light_sample_g<MIS, PICK, SAMPLE>(L, s, (double)n_lights));
}

// The plain form (rt_render_direct's estimator).
template <int THREADS, int MODE, int PICK, int SAMPLE>
__device__ __forceinline__ v3 direct_light(const DScene& S, const DNode4F* lds_nodes, const DPrim* lds_prims,
                                           const DLight* __restrict__ lights, int n_lights, Rng& rng, uint64_t seed,
                                           v3 x, v3 n, v3 a, unsigned* stk, unsigned& visits, unsigned& ptests,
                                           const typename PickGrid<PICK>::type& grid) {
  bool taken;
  int cell;
  return direct_light<THREADS, MODE, false, PICK, SAMPLE>(S, lds_nodes, lds_prims, lights, n_lights, rng, seed, x, n,
                                                          a, stk, visits, ptests, taken, grid, cell);
}

}  // namespace rt
