// portable_trig.h — the cosine that goes with portable_libm.h's pl_sin: the same reduction (k = rint(x 2/pi),
// r = x - k pi/2 in three Cody-Waite parts) and the same two kernels, taken in the cosine's quadrant order.
// Plain IEEE binary64 operations, so a CPU build and a gfx950 build (both -ffp-contract=off) return the same bits.
//
// Unlike portable_libm.h's diagnostic use, the product calls these: solid-angle sampling of rect lights
// (light_rect.h, include/shirley_rt.h) is defined on pl_sin, pl_cos and pl_acos, not on a libm.
#pragma once

#include "portable_libm.h"

PL_FN double pl_cos(double x) {
  if (!(fabs(x) <= 1e9)) return (x - x) * 0.0;  // NaN for inf / NaN; 0 beyond the reduction's range, as pl_sin
  const double invpio2 = 6.36619772367581382433e-01;
  const double p1 = 1.57079632673412561417e+00, p2 = 6.07710050630396597660e-11, p3 = 2.02226624871116645580e-21;
  const double k = rint(x * invpio2);
  const double r = ((x - k * p1) - k * p2) - k * p3;
  const double z = r * r;
  const double s = r + (r * z) * (-1.66666666666666324348e-01 +
                                  z * (8.33333333332248946124e-03 +
                                       z * (-1.98412698298579493134e-04 +
                                            z * (2.75573137070700676789e-06 +
                                                 z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))));
  const double c = (1.0 - 0.5 * z) + (z * z) * (4.16666666666666019037e-02 +
                                                z * (-1.38888888888741095749e-03 +
                                                     z * (2.48015872894767294178e-05 +
                                                          z * (-2.75573143513906633035e-07 +
                                                               z * (2.08757232129817482790e-09 +
                                                                    z * -1.13596475577881948265e-11)))));
  const int q = (int)((long long)k & 3);
  return q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
}
