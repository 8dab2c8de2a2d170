// light_rect.h — solid-angle sampling of an axis-aligned rect light (rt_scene_light_sampling, mode
// RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL; include/shirley_rt.h has the definition, operation for operation):
// the spherical rectangle a rect subtends from a vertex (Ureña, Fajardo and King 2013), its solid angle S, and the
// point of the rect that a uniform direction of it meets.
//
// One body for the device (direct.h, nee.hip) and for the host form rt_light_sample_host (rt_light_sample.cpp), like
// light_cone.h: plain binary64 with + - * /, a correctly rounded sqrt (cone_sqrt), comparisons and selects in the
// header's order, and pl_sin / pl_cos / pl_acos (portable_libm.h, portable_trig.h), which are such operations
// themselves.  The rect is axis-aligned, so its local frame is a permutation of the coordinates: the caller passes
// the vertex as (its d1 coordinate, its d2 coordinate, its coordinate along the rect's normal axis), and nothing
// is normalised.
#pragma once

#include "light_cone.h"
#include "portable_trig.h"

namespace rt {

constexpr int kSampleAll = 3;  // spheres as kSampleCone; rects: a uniform direction of their spherical rectangle

constexpr double kRectTwoPi = 6.283185307179586;
constexpr double kRectMinS = 0x1p-20;           // below it (or a NaN) the sample is the area form's
constexpr double kRectHvGuard = 1.0 - 0x1p-40;  // hv * hv at or above it: yv = y1

// What rect_open found.
constexpr int kRectCoplanar = 0;  // z0 == 0: the vertex lies in the rect's plane
constexpr int kRectSmall = 1;     // !(S >= 2^-20)
constexpr int kRectOpen = 2;

struct RectView {
  double x0, x1, y0, y1;  // the rect's bounds relative to the vertex
  double z0;              // its plane's offset relative to the vertex, negated where positive (z0 < 0)
  double b0, b1, k, S;
  bool flip;  // z0 was positive
};

// The spherical rectangle of the rect p = (d1_min, d1_max, d2_min, d2_max, offset) seen from (xd1, xd2, xa).
// kRectCoplanar leaves everything after z0 unset; kRectSmall and kRectOpen set it all.
RT_CONE_FN int rect_open(const double* p, double xd1, double xd2, double xa, RectView& v) {
  v.x0 = p[0] - xd1;
  v.x1 = p[1] - xd1;
  v.y0 = p[2] - xd2;
  v.y1 = p[3] - xd2;
  double z0 = p[4] - xa;
  v.z0 = z0;
  v.flip = false;
  if (z0 == 0.0) return kRectCoplanar;
  if (z0 > 0.0) {
    z0 = -z0;
    v.flip = true;
  }
  v.z0 = z0;
  const double zz = z0 * z0;
  // the z components of the four side planes' unit normals
  const double b0 = -v.y0 / cone_sqrt(zz + v.y0 * v.y0);
  const double n1z = v.x1 / cone_sqrt(zz + v.x1 * v.x1);
  const double b1 = v.y1 / cone_sqrt(zz + v.y1 * v.y1);
  const double n3z = -v.x0 / cone_sqrt(zz + v.x0 * v.x0);
  const double g0 = pl_acos(-(b0 * n1z));
  const double g1 = pl_acos(-(n1z * b1));
  const double g2 = pl_acos(-(b1 * n3z));
  const double g3 = pl_acos(-(n3z * b0));
  v.b0 = b0;
  v.b1 = b1;
  v.k = (kRectTwoPi - g2) - g3;
  v.S = (g0 + g1) - v.k;
  return v.S >= kRectMinS ? kRectOpen : kRectSmall;
}

// The point of an open view for the draws (u, v), relative to the vertex: (w1, w2) in the rect's plane along
// (d1, d2), wa along its normal axis.
RT_CONE_FN void rect_sample(const RectView& r, double u, double v, double& w1, double& w2, double& wa) {
  const double au = u * r.S + r.k;
  const double fu = (pl_cos(au) * r.b0 - r.b1) / pl_sin(au);
  double cu = 1.0 / cone_sqrt(fu * fu + r.b0 * r.b0);
  cu = fu > 0.0 ? cu : -cu;
  cu = cu < -1.0 ? -1.0 : cu > 1.0 ? 1.0 : cu;
  double xu = -(cu * r.z0) / cone_sqrt(1.0 - cu * cu);
  xu = xu < r.x0 ? r.x0 : xu > r.x1 ? r.x1 : xu;
  const double dd = xu * xu + r.z0 * r.z0;
  const double d = cone_sqrt(dd);
  const double h0 = r.y0 / cone_sqrt(dd + r.y0 * r.y0);
  const double h1 = r.y1 / cone_sqrt(dd + r.y1 * r.y1);
  const double hv = h0 + v * (h1 - h0);
  const double hv2 = hv * hv;
  w1 = xu;
  w2 = hv2 < kRectHvGuard ? (hv * d) / cone_sqrt(1.0 - hv2) : r.y1;
  wa = r.flip ? -r.z0 : r.z0;
}

}  // namespace rt
