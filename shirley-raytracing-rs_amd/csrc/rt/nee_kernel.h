// nee_kernel.h — nee_kernel, the one path body of rt_render_nee (nee.hip) and rt_render_nee_adaptive
// (nee_adaptive.hip): a path integrator that takes one light sample at every Lambertian / FairyLight vertex and
// weights the emission its scatter then lands on (include/shirley_rt.h).
//
// nee_kernel stands in the tile-pass frame (pass_frame.h: one wave per 8x8 tile, one lane per pixel, the block's
// LDS layout and placements, EXT = false) and runs whole paths in it by lane-level path regeneration: one
// wave-uniform loop whose iteration traces one segment per live lane with probe_kernel's body (trace.hip:
// traverse4, hit_record, the wave's marble_coop and draws_coop, shade_factor — the megakernel's device
// functions on the megakernel's draws), then applies the weight ws to the segment's emission and calls
// direct_light (direct.h) in the lanes whose vertex takes a light sample.  A lane whose path ended adds its
// radiance to its running pixel sum and starts its next sample in the next iteration, so a pixel's samples are
// added in order with no atomics and no inter-wave traffic.  Lanes outside the image and lanes out of samples
// stay in the loop, idle, for the wave-wide steps; the loop ends when the wave's last lane is done, and at the
// latest after (s_end - s_begin) * max_depth iterations — one segment per live lane per iteration cannot
// take more.  The light table and the primitive -> light table are kernel arguments of their own, and so is the
// light grid of a kPickGrid instance (light_pick.h, DESIGN.md §18: the argument `grid`, an empty record in the
// uniform instances), whose path state holds one more integer: the cell of the vertex that took the light sample.
// A kSampleCone instance (light_cone.h, DESIGN.md §19: rt_scene_light_sampling) samples sphere lights by solid
// angle and weights a listed sphere hit from the cone that sphere subtends at the segment's origin.  A kSampleAll
// instance (light_rect.h) does that and treats rects alike, by the spherical rectangle they subtend.
//
// An ADAPT instance (rt_render_nee_adaptive) is the same body under the stop rule of adaptive.h,
// applied by the wave that owns the tile.  Its grid is sized to the device, not to the frame: after the staging
// (the block's only barriers) each wave takes tiles from a counter until none is left, so no wave ever waits for
// another.  The lane's `sum` is the sum of the current batch (b samples); when the batch is complete the lane adds
// it to its pixel of `accum` and its y = (r + g) + b to the pixel's moments, in the output buffers (one owner per
// pixel: plain loads and stores).  s_to, the wave-uniform end of the current step, takes s_end's place in the
// loop: when the wave's last lane has reached it the wave computes the tile's error e (fold_stats_kernel's
// butterfly, trace.hip) and either moves s_to on by a step or writes e and the tile's count and fetches again.
#pragma once

#include <hip/hip_runtime.h>

#include "adaptive.h"
#include "direct.h"
#include "pass_frame.h"
#include "rt_launch.h"

namespace rt {

// The adaptive arguments (NeeAdapt, rt_launch.h): an empty record in the uniform instances, like
// PickGrid<PICK>::type.
struct NoNeeAdapt {};
template <bool ADAPT>
struct NeeAdaptArgs {
  typedef NoNeeAdapt type;
};
template <>
struct NeeAdaptArgs<true> {
  typedef NeeAdapt type;
};

// tile_lane's lane -> pixel mapping for a tile that the wave was handed
__device__ __forceinline__ TileLane tile_lane_of(int tile, int tiles_x) {
  const int lane = threadIdx.x % kWave;
  TileLane T;
  T.tile = tile;
  T.px = (tile % tiles_x) * kTile + lane % kTile;
  T.py = (tile / tiles_x) * kTile + lane / kTile;
  return T;
}

// A uniform instance (rt_render_nee) renders the tile of the wave -> tile map over [s_begin, s_end).  An ADAPT
// instance (rt_render_nee_adaptive; s_begin = 0, s_end = the per-pixel maximum) fetches tiles until the counter
// passes n_tiles, at most n_tiles times; no barrier follows the staging, so its waves leave on their own.  Its
// tile loop is the backward jump at the end of the body and not a loop statement around it: a statement of a
// single trip around this body already moves the uniform instances' register allocation (53 of the 60 change
// their spill counts), and those instances are to stay what they are.
template <int THREADS, int MODE, bool MIS, int PICK, int SAMPLE, bool ADAPT = false>
__global__ __launch_bounds__(THREADS) void nee_kernel(DScene S, DCamera C, uint64_t seed, int s_begin, int s_end,
                                                      int max_depth, int tiles_x, int n_tiles,
                                                      const DLight* __restrict__ lights, int n_lights,
                                                      const int32_t* __restrict__ prim_light,
                                                      double* __restrict__ accum,
                                                      const typename PickGrid<PICK>::type grid,
                                                      const typename NeeAdaptArgs<ADAPT>::type ad) {
  extern __shared__ unsigned char lds_raw[];
  const BlockLds<DNode4F> L = carve_block_lds<MODE, DNode4F>(S, lds_raw);
  stage_nodes4<MODE>(S, L.nodes, L.prims);
  int fetches = 0;  // ADAPT: tiles this wave has asked for (wave-uniform)
next_tile:
  TileLane T;
  if constexpr (ADAPT) {
    if (fetches++ >= n_tiles) return;
    unsigned t = 0u;
    if (threadIdx.x % kWave == 0) t = atomicAdd(ad.counter, 1u);
    t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
    if (t >= (unsigned)n_tiles) return;
    T = tile_lane_of((int)t, tiles_x);
  } else {
    T = tile_lane<THREADS>(tiles_x);
    if (T.tile >= n_tiles) return;
  }
  const bool active = T.active(C);
  const uint32_t pix = T.pix(C);
  unsigned visits = 0, ptests = 0;
#ifdef RT_PHASE_TIMING
  unsigned long long steps = 0;
#endif
  // the lane's path: sample s, segment k, ray (o, d), attenuation, radiance; prev / cx_prev: the last vertex
  // took a light sample, and the cosine of its scatter direction there; cell_prev: that vertex's cell of the
  // light grid (a kPickGrid instance's only)
  int s = s_begin, k = 1;
  bool fresh = true, prev = false;
  double cx_prev = 0.0;
  int cell_prev = 0;
  Rng rng{pix, (uint32_t)s_begin, 0u, 0u, 0u};
  v3 o = V(0.0, 0.0, 0.0), d = V(1.0, 1.0, 1.0);
  v3 att = V(1.0, 1.0, 1.0), rad = V(0.0, 0.0, 0.0), sum = V(0.0, 0.0, 0.0);
  // ADAPT: s_to, the end of the current step (wave-uniform; else the end of the call's range), and s_flush, the
  // sample count that completes the lane's current batch
  int s_to = s_end, s_flush = 0;
  if constexpr (ADAPT) {
    s_to = ad.min_samples;
    s_flush = ad.batch;
  }
  // one segment per live lane per iteration: no lane has more than `trips` of them (wave-uniform bound)
  const unsigned long long trips =
      (unsigned long long)(s_end > s_begin ? s_end - s_begin : 0) * (unsigned long long)(max_depth > 0 ? max_depth : 0);
  for (unsigned long long it = 0; it < trips; ++it) {
    const bool live = active && s < s_to;
    if (__ballot(live) == 0ull) break;  // wave-uniform: the wave's last lane is done
    if (live && fresh) {  // the next sample's camera ray (render.rs:60-63)
      rng = Rng{pix, (uint32_t)s, 0u, 0u, 0u};
      sample_ray(C, rng, seed, T.px, T.py, o, d);
      att = V(1.0, 1.0, 1.0);
      rad = V(0.0, 0.0, 0.0);
      k = 1;
      prev = false;
      fresh = false;
    }
    // probe_kernel's step 1: closest hit, record, material, texture leaf
    bool hit = false, need_pn = false, need_r = false;
    int prim = -1, face = -1, leaf = -1, mat = 0, ptab = 0, mk = -1;
    double t_best = __builtin_inf(), psc = 0.0;
    Hit h;
    h.point = V(0.0, 0.0, 0.0);
    h.normal = h.point;
    h.t = h.u = h.v = 0.0;
    h.front_face = false;
    if (live) {
      prim = traverse4<THREADS, MODE, false>(S, L.nodes, L.prims, o, d, 0.001, t_best, face, L.stk, rng, seed, visits,
                                             ptests RT_STAT_ARG(steps));
      if (prim >= 0) {
        hit = true;
        const DPrim pr = (MODE == kSceneLds) ? L.prims[prim] : S.prims[prim];
        hit_record<false, false>(S, pr, face, o, d, t_best, rng, seed, h);
        mat = pr.material;
        mk = S.mats[mat].kind;
        need_r = mk == RT_MAT_LAMBERTIAN || mk == RT_MAT_METAL || mk == RT_MAT_FAIRY_LIGHT || mk == RT_MAT_ISOTROPIC;
        if (mk == RT_MAT_LAMBERTIAN || mk == RT_MAT_FAIRY_LIGHT || mk == RT_MAT_DIFFUSE_LIGHT || mk == RT_MAT_ISOTROPIC)
          leaf = texture_leaf(S, S.mats[mat].tex, h.point, need_pn, ptab, psc);
      }
    }
    const bool ends = live && (!hit || mk == RT_MAT_DIFFUSE_LIGHT);
    // step 3: the wave's marble values and draws (every lane of the wave is here)
    const double pn = wave_marble(S, L.perlin, need_pn, ptab, psc, h.point);
    const bool scat = live && !ends;
    const int dk = (scat && need_r) ? kDrawSphere : (scat && mk == RT_MAT_DIELECTRIC) ? kDrawDiel : kDrawNone;
    double jx0 = 0.0, jy0 = 0.0;
    const v3 rs = draws_coop(rng, seed, dk, false, 0u, jx0, jy0);
    const v3 un = unit_fast(!live ? V(1.0, 1.0, 1.0) : (scat && need_r && mk != RT_MAT_METAL) ? rs : d);
    // step 4: emitted + scatter, or the sky; then the weight and the light sample
    if (live) {
      bool done = false;
      if (!hit) {
        rad = rad + hmul(att, sky_unit(S, un));  // a sky is never listed
        done = true;
      } else {
        const v3 din = d;  // the segment's direction (shade_factor replaces the ray)
        const v3 oin = o;  // ... and its origin, the previous vertex (read by the solid-angle instances only)
        bool has_emit = false;
        v3 mul = V(1.0, 1.0, 1.0), emit = V(0.0, 0.0, 0.0);
        const bool alive = shade_factor(S, S.texs, S.mats[mat], leaf, pn, rs, un, rng, o, d, h, prim, face, mul, emit,
                                        has_emit);
        if (has_emit) {
          double ws = 1.0;
          const int lj = prev ? prim_light[prim] : -1;
          if (lj >= 0 && (lights[lj].geometry != RT_GEOM_SPHERE || h.front_face)) {
            // kSampleAll, a rect: its spherical rectangle at the previous vertex by the light sample's own rule
            // (kRectSmall: the area-measure weight below; kRectCoplanar, or !(cx_prev > 0): ws stays 1)
            int rect_w = kRectSmall;
            double rect_S = 0.0;
            if constexpr (SAMPLE == kSampleAll) {
              const DLight& Lj = lights[lj];
              const int gj = Lj.geometry;
              if (gj != RT_GEOM_SPHERE) {
                RectView rv;
                rect_w = rect_open(Lj.p, gj == RT_GEOM_RECT_YZ ? oin.y : oin.x, gj == RT_GEOM_RECT_XY ? oin.y : oin.z,
                                   gj == RT_GEOM_RECT_XY ? oin.z : gj == RT_GEOM_RECT_YZ ? oin.x : oin.y, rv);
                if (!(cx_prev > 0.0)) rect_w = kRectCoplanar;
                if (rect_w == kRectOpen) rect_S = rv.S;
              }
            }
            if (SAMPLE == kSampleAll && rect_w != kRectSmall) {
              if (rect_w == kRectOpen) {
                if (MIS) {
                  const double gs = cx_prev / kDirectPi;
                  double pl;
                  if constexpr (PICK == kPickGrid)
                    pl = light_prob(grid, cell_prev, n_lights, lj) / rect_S;
                  else
                    pl = 1.0 / (rect_S * (double)n_lights);
                  ws = gs / (pl + gs);
                } else {
                  ws = 0.0;
                }
              }
            } else if (SAMPLE != kSampleArea && lights[lj].geometry == RT_GEOM_SPHERE) {
              // both densities per solid angle at the previous vertex: the scatter's cx_prev / pi, the light
              // sample's 1 / (2 pi om) per pick; from inside the sphere the light sample gave nothing
              const DLight& Lj = lights[lj];
              c3 wc;
              double dc2, om;
              if (cone_open(c3{Lj.p[0], Lj.p[1], Lj.p[2]}, Lj.p[3], c3{oin.x, oin.y, oin.z}, wc, dc2, om) &&
                  cx_prev > 0.0) {
                if (MIS) {
                  const double gs = cx_prev / kDirectPi;
                  double pl;
                  if constexpr (PICK == kPickGrid)
                    pl = light_prob(grid, cell_prev, n_lights, lj) / ((2.0 * kDirectPi) * om);
                  else
                    pl = 1.0 / (((2.0 * kDirectPi) * om) * (double)n_lights);
                  ws = gs / (pl + gs);
                } else {
                  ws = 0.0;
                }
              }
            } else if (MIS) {
              const double ld2 = (din.x * din.x + din.y * din.y) + din.z * din.z;
              const double ld = sqrt_rn(ld2);
              const double cy = -dot(h.normal, din) / ld;
              const double d2 = (h.t * h.t) * ld2;
              if (cx_prev > 0.0 && cy > 0.0) {
                const double gs = ((cx_prev * cy) / d2) / kDirectPi;
                double pl;
                if constexpr (PICK == kPickGrid)
                  pl = light_prob(grid, cell_prev, n_lights, lj) / lights[lj].area;
                else
                  pl = 1.0 / (lights[lj].area * (double)n_lights);
                ws = gs / (pl + gs);
              }
            } else {
              ws = 0.0;
            }
          }
          rad = rad + scale(hmul(att, emit), ws);
        }
        if (!alive) {
          done = true;
        } else {
          prev = false;
          if ((mk == RT_MAT_LAMBERTIAN || mk == RT_MAT_FAIRY_LIGHT) && n_lights > 0 && k < max_depth) {
            // on the path's draws after the scatter's own; stands for segment k + 1's emission
            const v3 dl = direct_light<THREADS, MODE, MIS, PICK, SAMPLE>(S, L.nodes, L.prims, lights, n_lights, rng,
                                                                         seed, h.point, h.normal, mul, L.stk, visits,
                                                                         ptests, prev, grid, cell_prev);
            rad = rad + hmul(att, dl);
            cx_prev = dot(h.normal, d) / sqrt_rn(len2(d));
          }
          att = hmul(att, mul);
          ++k;
          done = k > max_depth;
        }
      }
      if (done) {  // the sample's value is rad; the lane's next sample starts in the next iteration
        sum = sum + rad;
        ++s;
        fresh = true;
        if constexpr (ADAPT) {
          if (s == s_flush) {  // the batch is complete: fold_stats_kernel's additions, from 0 for the first batch
            const size_t p = (size_t)T.py * (size_t)C.width + (size_t)T.px;
            const bool first = s == ad.batch;
            const double y = (sum.x + sum.y) + sum.z;
            accum[p * 3 + 0] = (first ? 0.0 : accum[p * 3 + 0]) + sum.x;
            accum[p * 3 + 1] = (first ? 0.0 : accum[p * 3 + 1]) + sum.y;
            accum[p * 3 + 2] = (first ? 0.0 : accum[p * 3 + 2]) + sum.z;
            ad.moments[p * 2 + 0] = (first ? 0.0 : ad.moments[p * 2 + 0]) + y;
            ad.moments[p * 2 + 1] = fma(y, y, first ? 0.0 : ad.moments[p * 2 + 1]);
            sum = V(0.0, 0.0, 0.0);
            s_flush += ad.batch;
          }
        }
      }
    }
    if constexpr (ADAPT) {
      if (__ballot(active && s < s_to) == 0ull) {  // wave-uniform: the step is rendered, the tile's check
        const size_t p = (size_t)T.py * (size_t)C.width + (size_t)T.px;
        const long long n = s_to / ad.batch;
        double E = 0.0, M = 0.0;
        int K = 0;
        if (active) {
          M = ad.moments[p * 2 + 0];
          E = pixel_variance(M, ad.moments[p * 2 + 1], n);
          K = 1;
        }
        for (int off = kWave / 2; off > 0; off >>= 1) {
          E += __shfl_xor(E, off);
          M += __shfl_xor(M, off);
          K += __shfl_xor(K, off);
        }
        const double e = tile_error(E, M, K, n, ad.batch, ad.noise_floor);
        // (every lane holds the same e; the ballot makes the branch, and with it s_to, wave-uniform by construction)
        if (__ballot(tile_continues(e, ad.threshold) && s_to < s_end) != 0ull) {
          s_to = s_end - s_to <= ad.step ? s_end : s_to + ad.step;
        } else {
          if (threadIdx.x % kWave == 0 && ad.tile_err) ad.tile_err[T.tile] = e;
          if (active) ad.counts[p] = s_to;
          break;
        }
      }
    }
  }
  if constexpr (!ADAPT) {
    if (!active) return;
    const size_t p = (size_t)T.py * (size_t)C.width + (size_t)T.px;
    accum[p * 3 + 0] = sum.x;
    accum[p * 3 + 1] = sum.y;
    accum[p * 3 + 2] = sum.z;
  }
  if constexpr (ADAPT) goto next_tile;
}

// The instance of (placement T x M, ADAPT) that the scene's settings select: go(kernel, grid record).  `grid`
// (null: the uniform pick) is read only where n_lights > 0; `sample`: kSampleArea, kSampleCone or kSampleAll.
template <int T, int M, bool ADAPT, class Go>
hipError_t nee_instance(bool mis, const DLightGrid* grid, int n_lights, int sample, Go go) {
  auto pick = [&](auto kind) {
    constexpr int SM = decltype(kind)::value;
    if (grid && n_lights > 0)
      return mis ? go(nee_kernel<T, M, true, kPickGrid, SM, ADAPT>, *grid)
                 : go(nee_kernel<T, M, false, kPickGrid, SM, ADAPT>, *grid);
    return mis ? go(nee_kernel<T, M, true, kPickUniform, SM, ADAPT>, NoLightGrid{})
               : go(nee_kernel<T, M, false, kPickUniform, SM, ADAPT>, NoLightGrid{});
  };
  return sample == kSampleAll    ? pick(std::integral_constant<int, kSampleAll>{})
         : sample == kSampleCone ? pick(std::integral_constant<int, kSampleCone>{})
                                 : pick(std::integral_constant<int, kSampleArea>{});
}

}  // namespace rt
