// occlusion.h — any-hit traversal of the render tree (include/shirley_rt.h, ABI 11).
//
// occluded4 answers "does traverse4 with the same (o, d, t_min, t_max) return a primitive?" without the
// closest-hit bookkeeping: t_max is never shrunk, the walk ends on the first accepted leaf, and nothing marks
// or resolves ties.  The accept decisions are traverse4's own, in their arithmetic: its prologue, node4_visit
// for the f32 keys and the hit-leaf mask, and leaf_tests4's three loops (occ_leaves4, a copy without
// tie_takes / mark_tie that returns on the first accept; the sphere, rect and RectBox tests are the functions
// leaf_tests4 calls).  Why the answers agree exactly: every leaf test is a pure function of (ray, t_min,
// t_max') and monotone in t_max' — a primitive accepted at a shrunken t_best is accepted at the full t_max,
// and where one is accepted at the full t_max the closest-hit walk, which reaches that leaf with t_best <
// t_max only after another accept, ends with some hit.  The conservative node tests keep every subtree that
// holds such a leaf, at the constant bound as at a shrunken one.
// Reference scenes only (EXT = false, DNode4F); included by occlusion.hip alone.
#pragma once

#include "rt_device.h"

// RT_OCC_UNSORTED (a compile-time A/B): 1 pushes the surviving internal children in child
// order, without node4_next's sorting network; 0 keeps node4_next unchanged.  Measured on ~10^6 bounce rays
// (profiles/occlusion/measure.json): sorted, the any-hit walk beats traverse4 by 10-17 % on the headline
// scene and loses 4-6 % on Cornell, where nearly every wave holds an unoccluded ray that walks the whole
// tree; unsorted it keeps 8-15 % of the headline gain and is level with or ahead of traverse4 on Cornell.
// The instance that is not slower on both batches is the default.
#ifndef RT_OCC_UNSORTED
#define RT_OCC_UNSORTED 1
#endif

namespace rt {

// leaf_tests4<MODE, false>'s loops against the constant bound t_max: true on the first accepted leaf.
template <int MODE>
__device__ __forceinline__ bool occ_leaves4(const DScene& S, const DPrim* lds_prims, v3 o, v3 d, v3 inv, RaySigns ns,
                                            const Recip& ra, bool ra_ok, double t_min, double t_max, unsigned lm,
                                            int c0, int c1, int c2, int c3, const int32_t* chp, unsigned& ptests) {
  const unsigned nf = ~top_bytes((unsigned)c0, (unsigned)c1, (unsigned)c2, (unsigned)c3);
  const unsigned gm = (nf << 2) & 0x80808080u, bm = (nf << 3) & 0x80808080u;
  unsigned sph = lm & ~gm, rect = lm & gm & ~bm, box = lm & bm;
  const bool div_ok = ra_ok;
  constexpr bool kReread = MODE == kNodesLds || MODE == kSceneLds;
  auto child = [&](int k) -> int { return kReread ? chp[k] : child_at(k, c0, c1, c2, c3); };
#pragma unroll 1
  while (sph) {
    const int k = __builtin_ctz(sph) >> 3;
    sph &= sph - 1;
    const int leaf = ~child(k);
    const DPrim& pr = (MODE == kSceneLds) ? lds_prims[leaf] : S.prims[leaf];
    double t;
    RT_STAT(++ptests);
    bool sure;
    if (!sphere_t_sure(pr.p, o, d, ra, ra_ok, t_min, t_max, t, sure)) continue;
    if (sure || slab_sphere(pr.p, o, inv, ns, t_min, t_max)) return true;
  }
#pragma unroll 1
  while (box) {
    const int k = __builtin_ctz(box) >> 3;
    box &= box - 1;
    const int leaf = (~child(k)) & kLeafPrimMask;
    const DPrim& pr = (MODE == kSceneLds) ? lds_prims[leaf] : S.prims[leaf];
    constexpr bool kTwoPass = (RT_BOX_TWO_PASS & 1) != 0;
    constexpr bool kOneFull = (RT_BOX_TWO_PASS & 4) != 0 && MODE == kSceneLds;
    double te, tx, t;
    if (!slab_s(pr.p, o, inv, ns, t_min, t_max, te, tx)) continue;
    RT_STAT(++ptests);
    const int f = (kTwoPass && div_ok)   ? box_t2(pr.p, o, d, inv, ns, t_min, t_max, te, tx, t)
                  : (kOneFull && div_ok) ? box_t1f(pr.p, o, d, inv, ns, t_min, t_max, te, tx, t)
                                         : box_t(pr.p, o, d, t_min, t_max, t, inv, div_ok);
    if (f >= 0) return true;
  }
#pragma unroll 1
  while (rect) {
    const int k = __builtin_ctz(rect) >> 3;
    rect &= rect - 1;
    const int leaf = (~child(k)) & kLeafPrimMask;
    const DPrim& pr = (MODE == kSceneLds) ? lds_prims[leaf] : S.prims[leaf];
    double b[6], te, t;
    leaf_box(pr, b);
    if (!slab_s(b, o, inv, ns, t_min, t_max, te)) continue;
    RT_STAT(++ptests);
    bool h;
    switch (pr.kind) {
      case kPrimRectXY: h = rect_t<0, 1>(pr.p, o, d, t_min, t_max, t, inv, div_ok); break;
      case kPrimRectYZ: h = rect_t<1, 2>(pr.p, o, d, t_min, t_max, t, inv, div_ok); break;
      default: h = rect_t<0, 2>(pr.p, o, d, t_min, t_max, t, inv, div_ok);
    }
    if (h) return true;
  }
  return false;
}

// node4_next without the sorting network: the internal children that pass the cull are pushed in child
// order (at most three; the first survivor is the next node).  The bound never shrinks, so no pushed entry
// is ever culled later and a pop is one read.
template <int STRIDE>
__device__ __forceinline__ int occ_next_unsorted(const DScene& S, int4 ch, float k0, float k1, float k2, float k3,
                                                 float tmaxf, int& sp, unsigned& top, unsigned* stk) {
  const unsigned km = S.key_mask;
  const unsigned p0 = (__float_as_uint(k0) & ~km) | (unsigned)ch.x;
  const unsigned p1 = (__float_as_uint(k1) & ~km) | (unsigned)ch.y;
  const unsigned p2 = (__float_as_uint(k2) & ~km) | (unsigned)ch.z;
  const unsigned p3 = (__float_as_uint(k3) & ~km) | (unsigned)ch.w;
  const unsigned lim = __float_as_uint(tmaxf) | km;
  unsigned next = ~0u;
  auto take = [&](unsigned p) {
    if (p > lim) return;
    if (next != ~0u) { stk[sp] = top; sp += STRIDE; top = next; }
    next = p;
  };
  take(p3);
  take(p2);
  take(p1);
  take(p0);
  if (next != ~0u) return (int)(next & km);
  const unsigned e = top;
  if (e == ~0u) return -1;
  sp -= STRIDE;
  top = stk[sp];
  return (int)(e & km);
}

// True iff traverse4<STRIDE, MODE, false> with the same (o, d, t_min, t_max) returns a primitive.
template <int STRIDE, int MODE>
__device__ __forceinline__ bool occluded4(const DScene& S, const DNode4F* lds_nodes, const DPrim* lds_prims, v3 o, v3 d,
                                          double t_min, double t_max, unsigned* stk, unsigned& visits,
                                          unsigned& ptests) {
  // traverse4's prologue
  bool inv_ok;
  const v3 inv = inv_dir(d, inv_ok);
  const RaySigns ns = ray_signs(inv);
  const RayF rf = ray_f<DNode4F>(S, o, inv);
  const double a = len2(d);
  const Recip ra = recip(a);
  const bool ra_ok = inv_ok && a >= 0x1p-300 && a <= 0x1p300 && rf.fast && t_min >= 0.001;
  const float tmaxf = tmax_f32(t_max);
  int sp = 0;
  unsigned top = ~0u;
  int node = S.root4;
  // (traverse4's guard: more steps than nodes can only be a defect, and ends the loop)
  for (int steps = 0; steps < S.n_nodes4 && node >= 0; ++steps) {
    int4 ch;
    float k0, k1, k2, k3;
    const int32_t* chp;
    const unsigned lm = node4_visit<MODE>(S, lds_nodes, o, inv, rf, t_min, t_max, tmaxf, node, ch, k0, k1, k2, k3,
                                          visits, chp);
    if (lm && occ_leaves4<MODE>(S, lds_prims, o, d, inv, ns, ra, ra_ok, t_min, t_max, lm, ch.x, ch.y, ch.z, ch.w, chp,
                                ptests))
      return true;
#if RT_OCC_UNSORTED
    node = occ_next_unsorted<STRIDE>(S, ch, k0, k1, k2, k3, tmaxf, sp, top, stk);
#else
    node = node4_next<STRIDE, MODE != kSceneLds>(S, ch, k0, k1, k2, k3, tmaxf, sp, top, stk);
#endif
  }
  return false;
}

}  // namespace rt
