// light_cone.h — solid-angle sampling of a sphere light (rt_scene_light_sampling; include/shirley_rt.h has the
// definition, operation for operation): the cone a sphere subtends from a vertex, the direction
// of a disk point in it, and the point of the sphere that direction meets first.
//
// One body for the device (direct.h, nee.hip) and for the host form rt_light_sample_host (rt_light_sample.cpp):
// plain binary64 with only + - * /, a correctly rounded sqrt, comparisons and selects in the header's order
// (both builds compile with -ffp-contract=off).  The kernels take their sqrt from sqrt_rn (rt_device.h), the
// host form from the compiler's.
#pragma once

#if defined(__HIPCC__)
#define RT_CONE_FN __host__ __device__ __forceinline__  // (a call would keep its reference results in scratch)
#else
#define RT_CONE_FN inline
#endif

namespace rt {

// The sample kind: a template parameter of direct_light, direct_kernel and nee_kernel (RT_LIGHT_SAMPLE_*).
constexpr int kSampleArea = 0;   // a uniform point of the light's area
constexpr int kSampleCone = 1;   // sphere lights: a uniform direction of the cone the sphere subtends

struct c3 {
  double x, y, z;
};

// (direct.h sets RT_CONE_SQRT to sqrt_rn before it includes this file)
#ifndef RT_CONE_SQRT
#define RT_CONE_SQRT __builtin_sqrt
#endif
RT_CONE_FN double cone_sqrt(double v) { return RT_CONE_SQRT(v); }

// The cone of the sphere (c, r) seen from x: wc = c - x, dc2 = |wc|^2, and om = 1 - cos(theta_max) without
// cancellation.  False from inside or on the sphere (!(dc2 > r*r), a NaN too): om is then not set.
RT_CONE_FN bool cone_open(c3 c, double r, c3 x, c3& wc, double& dc2, double& om) {
  wc = c3{c.x - x.x, c.y - x.y, c.z - x.z};
  dc2 = (wc.x * wc.x + wc.y * wc.y) + wc.z * wc.z;
  if (!(dc2 > r * r)) return false;
  const double s2 = (r * r) / dc2;
  const double cm = cone_sqrt(1.0 - s2);
  om = s2 / (1.0 + cm);
  return true;
}

// The sample of an open cone for the disk point (px, py), px*px + py*py <= 1: w = the vector from x to the
// point of the sphere that the direction meets first, u = that point's unit normal.
RT_CONE_FN void cone_sample(c3 c, double r, c3 x, c3 wc, double dc2, double om, double px, double py, c3& w,
                            c3& u) {
  const double dc = cone_sqrt(dc2);
  const c3 a{wc.x / dc, wc.y / dc, wc.z / dc};
  // the axis's orthonormal basis (t1, t2, a): |sg + a.z| >= 1 always
  const double sg = a.z < 0.0 ? -1.0 : 1.0;
  const double A = -1.0 / (sg + a.z);
  const double B = (a.x * a.y) * A;
  const c3 t1{1.0 + ((sg * a.x) * a.x) * A, sg * B, -(sg * a.x)};
  const c3 t2{B, sg + (a.y * a.y) * A, -a.y};
  // q is uniform on [0, 1] and independent of the disk point's angle: ct = cos(theta) uniform on [1 - om, 1]
  const double q = px * px + py * py;
  const double e = q * om;
  const double ct = 1.0 - e;
  const double k = cone_sqrt(om * (1.0 + ct));
  const double k1 = px * k, k2 = py * k;
  const c3 omega{(t1.x * k1 + t2.x * k2) + a.x * ct, (t1.y * k1 + t2.y * k2) + a.y * ct,
                 (t1.z * k1 + t2.z * k2) + a.z * ct};
  const double st2 = e * (1.0 + ct);
  double disc = r * r - dc2 * st2;
  disc = disc > 0.0 ? disc : 0.0;
  const double ds = dc * ct - cone_sqrt(disc);
  w = c3{omega.x * ds, omega.y * ds, omega.z * ds};
  u = c3{((x.x + w.x) - c.x) / r, ((x.y + w.y) - c.y) / r, ((x.z + w.z) - c.z) / r};
}

}  // namespace rt
