/* CPU check of the serve body written out for a y face (rt_device.h serve_y): for a dielectric hit on
 * face 4 or 5 of a RectBox the hop passes of the HOP = 4 instances form the record and the scattered ray with the axis
 * normal (0, +-1, 0) written out — front face from the sign of d.y, cos_theta = fmin(|ud.y|, 1), reflection (ud.x, -ud.y,
 * ud.z), refraction with the normal's terms kept for y alone — and hand every lane with a zero or tiny component
 * (min |d_i| < 2^-300, |d| > 2^300, ratio < 2^-400) to the general body.  Every output bit must be the general
 * body's: the new origin, the new direction, and whether the uniform was consumed (which is what moves rng.draw,
 * rng.c2 and rng.c3; the depth count and the death decision follow the segment, not its arithmetic).
 *
 * The general body is restated from the oracle's own functions (oracle.c, included unchanged: make_hit, ray_at,
 * vunit, or_fmin, reflectance, reflect, refract) as material_scatter's dielectric branch applies them, with the
 * uniform passed in; the reduced form is restated below from those functions' definitions, not taken from the kernel.
 *
 *   serve_y_check <cases per index> [seed]
 * Indices 1.0, 1.3, 1/1.3, 1.5, 1/1.5; per case a face (4, 5), a side (d.y < 0, > 0) and one of the families:
 *   0 a random direction at a random length 2^-300 .. 2^300     1 d.x, d.z, or both +-0
 *   2 d.x or d.z so small that ud underflows to +-0 or is subnormal
 *   3 normal incidence, ud.y = -+1 exactly, also with tiny and zero side components
 *   4 grazing, |ud.y| from 1e-2 down to 1e-7 (random_scene's dy_min is 9.2e-4)
 *   5 |d| at and beyond both ends of unit_fast's range, 2^+-290 .. 2^+-320
 *   6 cos_theta within a few ulps either side of total internal reflection's threshold sqrt(1 - 1 / ratio^2)
 *   7 as 0, with the uniform set to the reflectance, and to the values an ulp either side of it
 * Prints one JSON line and exits 1 when an output differs.  Two controls are counted and reported, not asserted:
 * `control_no_zero_rule` — the reduced form applied to every lane, fallback off — and `control_no_fmin` — cos_theta =
 * |ud.y| without the minimum.  Found (2 M cases per index): the first differs on about one case in ten (the sign
 * of a zero component of the new direction, or of the reflection of ud.y = +-0: 977 235 of 10 M); the second differs on
 * none (0 of 10 M, with 2.2 M cases at |ud.y| = 1 exactly): |d| = RN(sqrt(s)) with s >= RN(d.y^2) — rounding and adding
 * non-negative terms are monotone — and sqrt(RN(y^2)) is within a quarter ulp of |y|, so it rounds to |y|; hence
 * |d| >= |d.y| and |ud.y| <= 1 whenever the square does not underflow, which the range test excludes.  Inside the
 * reduced form's range the minimum is an identity; it is kept as the general body writes it (one v_min_f64 with the
 * |.| modifier on the device).  Test infrastructure (tests/test_serve_y.py); -ffp-contract=off. */
#include "../oracle/oracle.c"

#include <stdio.h>

static uint64_t s_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64(void) {
  uint64_t x = s_state;
  x ^= x << 13; x ^= x >> 7; x ^= x << 17;
  return s_state = x;
}
static double unif(void) { return (double)(next_u64() >> 11) * 0x1p-53; }
static double range(double a, double b) { return a + (b - a) * unif(); }
static double sgn(void) { return (next_u64() & 1) ? 1.0 : -1.0; }
static double ulps(double x, int k) {
  for (; k > 0; --k) x = nextafter(x, INFINITY);
  for (; k < 0; ++k) x = nextafter(x, -INFINITY);
  return x;
}
static uint64_t bits(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }

typedef struct out_t {
  v3 o, d;
  int drew;  /* the uniform was consumed: rng.draw + 1, rng.c2 / c3 from the cache */
  int refl, tir;
} out_t;

/* hit_record + unit + dielectric.rs:21-49 on a y face, from the oracle's functions (rect_hit's record for n = 1) */
static out_t general(const ray_t* r, double t, double ir, double u) {
  const hit_t h = make_hit(r, ray_at(r, t), V(0.0, 1.0, 0.0), t, 0.0, 0.0);
  const double ratio = h.front_face ? (1.0 / ir) : ir;
  const v3 ud = vunit(r->d);
  const double cos_theta = or_fmin(vdot(vscale(ud, -1.0), h.normal), 1.0);
  const double sin_theta = sqrt(1.0 - cos_theta * cos_theta);
  out_t q;
  q.tir = ratio * sin_theta > 1.0;
  q.drew = !q.tir;
  q.refl = q.tir || reflectance(cos_theta, ratio) > u;
  q.o = h.point;
  q.d = q.refl ? reflect(ud, h.normal) : refract(ud, h.normal, ratio);
  return q;
}

/* serve_y, restated.  zero_rule 0: no fallback (control); use_fmin 0: cos_theta = |ud.y| (control).  Returns 0 when
 * the lane falls back to the general body. */
static int reduced(const ray_t* r, double t, double ir, double u, int zero_rule, int use_fmin, out_t* q) {
  const v3 d = r->d;
  const double n = vlen(d);
  const double mn = fmin(fmin(fabs(d.x), fabs(d.y)), fabs(d.z));
  const int front = d.y < 0.0;
  const double ratio = front ? (1.0 / ir) : ir;
  if (zero_rule && !(mn >= 0x1p-300 && n <= 0x1p300 && ratio >= 0x1p-400)) return 0;
  const v3 ud = V(d.x / n, d.y / n, d.z / n);
  const double a = fabs(ud.y);
  const double cos_theta = use_fmin ? ((a < 1.0) ? a : 1.0) : a;
  q->tir = ratio > 1.0 && ratio * sqrt(1.0 - cos_theta * cos_theta) > 1.0;
  q->drew = !q->tir;
  q->refl = q->tir || reflectance(cos_theta, ratio) > u;
  q->o = vadd(r->o, vscale(d, t));
  if (q->refl) {
    q->d = V(ud.x, -ud.y, ud.z);
  } else {
    const double px = ud.x * ratio, pz = ud.z * ratio;
    const double py = ((front ? cos_theta : -cos_theta) + ud.y) * ratio;
    const double mag = sqrt(fabs(1.0 - ((px * px + py * py) + pz * pz))) * -1.0;
    q->d = V(px, py + (front ? mag : -mag), pz);
  }
  return 1;
}

static int same(const out_t* a, const out_t* b) {
  return bits(a->o.x) == bits(b->o.x) && bits(a->o.y) == bits(b->o.y) && bits(a->o.z) == bits(b->o.z) &&
         bits(a->d.x) == bits(b->d.x) && bits(a->d.y) == bits(b->d.y) && bits(a->d.z) == bits(b->d.z) && a->drew == b->drew;
}
/* (a NaN direction compares by its bits too: both forms reach it through the same operations or not at all) */

static double tiny(void) {  /* magnitudes that make ud.x underflow or come out subnormal against |d| ~ 1 */
  switch (next_u64() % 5) {
    case 0: return 0x1p-1074 * (double)(1 + next_u64() % 7);
    case 1: return ldexp(range(1.0, 2.0), -1074 + (int)(next_u64() % 60));
    case 2: return ldexp(range(1.0, 2.0), -1022 - (int)(next_u64() % 4));
    case 3: return ldexp(range(1.0, 2.0), -1022 + (int)(next_u64() % 4));
    default: return ldexp(range(1.0, 2.0), -301 + (int)(next_u64() % 3));  /* either side of 2^-300 */
  }
}

#define FAMILIES 8

int main(int argc, char** argv) {
  const long per = argc > 1 ? atol(argv[1]) : 2000000;
  if (argc > 2) s_state ^= (uint64_t)atoll(argv[2]) * 0xD1342543DE82EF95ull;
  const double irs[5] = {1.0, 1.3, 1.0 / 1.3, 1.5, 1.0 / 1.5};
  long cases = 0, wrong = 0, fell_back = 0, took = 0, n_tir = 0, n_refl = 0, n_refr = 0, c_zero = 0, c_fmin = 0, zero_comp = 0,
       cos_one = 0, fam_n[FAMILIES] = {0}, side_face[2][2] = {{0}};
  for (int ii = 0; ii < 5; ++ii) {
    const double ir = irs[ii];
    for (long k = 0; k < per; ++k) {
      const int fam = (int)(k % FAMILIES), face = 4 + (int)((k / FAMILIES) & 1), down = (int)((k / (2 * FAMILIES)) & 1);
      const double sy = down ? -1.0 : 1.0;
      const double ratio = down ? 1.0 / ir : ir;
      v3 d = V(range(-1.0, 1.0), sy * range(0.05, 1.0), range(-1.0, 1.0));
      double u = unif();
      switch (fam) {
        case 0:
        case 7:
          d = vscale(d, ldexp(1.0, (int)(next_u64() % 601) - 300));
          break;
        case 1: {
          const int w = 1 + (int)(next_u64() % 3);
          if (w & 1) d.x = 0.0 * sgn();
          if (w & 2) d.z = 0.0 * sgn();
          if (next_u64() & 1) d = vscale(d, ldexp(1.0, (int)(next_u64() % 401) - 200));
          break;
        }
        case 2: {
          const int w = 1 + (int)(next_u64() % 3);
          if (w & 1) d.x = tiny() * sgn();
          if (w & 2) d.z = tiny() * sgn();
          if (next_u64() % 4 == 0) d.y = sy * ldexp(range(1.0, 2.0), (int)(next_u64() % 40));  /* ... or is pushed under by a long d.y */
          break;
        }
        case 3: {
          const int w = (int)(next_u64() % 4);
          d.y = sy * ((next_u64() & 1) ? ldexp(1.0, (int)(next_u64() % 41) - 20) : range(0.5, 4.0));
          d.x = w == 0 ? 0.0 * sgn() : w == 1 ? tiny() * sgn() : d.y * ldexp(range(-1.0, 1.0), -27 - (int)(next_u64() % 30));
          d.z = w == 0 ? 0.0 * sgn() : w == 2 ? tiny() * sgn() : d.y * ldexp(range(-1.0, 1.0), -27 - (int)(next_u64() % 30));
          break;
        }
        case 4:
          d.y = sy * exp(range(log(1e-7), log(1e-2)));
          if (next_u64() & 1) d = vscale(d, ldexp(1.0, (int)(next_u64() % 201) - 100));
          break;
        case 5: {
          const int e = 290 + (int)(next_u64() % 31);
          d = vscale(d, ldexp(1.0, (next_u64() & 1) ? e : -e));
          break;
        }
        case 6: {
          if (ratio > 1.0) {  /* cos_theta around the threshold: ud.y = -+c, the side components share sqrt(1 - c^2) */
            const double c = ulps(sqrt(1.0 - 1.0 / (ratio * ratio)), (int)(next_u64() % 9) - 4);
            const double s = sqrt(1.0 - c * c), phi = range(0.0, 6.283185307179586);
            d = V(s * cos(phi), sy * c, s * sin(phi));
            if (next_u64() & 1) d = vscale(d, range(0.5, 2.0));
          } else {  /* no threshold on this side: angles across the whole range instead */
            const double c = unif(), s = sqrt(1.0 - c * c), phi = range(0.0, 6.283185307179586);
            d = V(s * cos(phi), sy * fmax(c, 1e-9), s * sin(phi));
          }
          break;
        }
      }
      /* the ray starts off the face and meets it at the correctly rounded quotient, as the passes' t is */
      const double yf = face == 4 ? 0.0 : -0.0078125;
      ray_t r;
      r.d = d;
      r.o = V(range(-4.0, 4.0), yf - sy * range(0.001, 0.5), range(-4.0, 4.0));
      if (next_u64() % 8 == 0) r.o.x = 0.0 * sgn();
      const double t = (yf - r.o.y) / d.y;
      if (fam == 7) {
        const out_t g0 = general(&r, t, ir, 2.0);
        if (!g0.tir) {
          const v3 ud = vunit(d);
          const double R = reflectance(or_fmin(fabs(ud.y), 1.0), ratio);
          u = ulps(R, (int)(next_u64() % 3) - 1);
        }
      }
      const out_t g = general(&r, t, ir, u);
      out_t q = g, c1, c2;
      const int by_y = reduced(&r, t, ir, u, 1, 1, &q);
      ++cases;
      ++fam_n[fam];
      ++side_face[down][face - 4];
      by_y ? ++took : ++fell_back;
      n_tir += g.tir;
      n_refl += g.refl && !g.tir;
      n_refr += !g.refl;
      zero_comp += (g.d.x == 0.0) + (g.d.z == 0.0);
      { const v3 ud = vunit(d); cos_one += fabs(ud.y) >= 1.0; }
      if (!same(&g, &q)) {
        if (++wrong <= 5)
          fprintf(stderr, "differs: ir %a fam %d d %a %a %a t %a u %a: general d %a %a %a drew %d, reduced d %a %a %a drew %d\n", ir,
                  fam, d.x, d.y, d.z, t, u, g.d.x, g.d.y, g.d.z, g.drew, q.d.x, q.d.y, q.d.z, q.drew);
      }
      reduced(&r, t, ir, u, 0, 1, &c1);
      c_zero += !same(&g, &c1);
      if (!reduced(&r, t, ir, u, 1, 0, &c2)) c2 = g;
      c_fmin += !same(&g, &c2);
    }
  }
  printf("{\"cases\": %ld, \"per_index\": %ld, \"wrong\": %ld, \"reduced\": %ld, \"fell_back\": %ld, \"tir\": %ld, "
         "\"reflected\": %ld, \"refracted\": %ld, \"zero_components_out\": %ld, \"cos_at_or_above_one\": %ld, "
         "\"control_no_zero_rule\": %ld, \"control_no_fmin\": %ld, \"families\": [%ld, %ld, %ld, %ld, %ld, %ld, %ld, %ld], "
         "\"up_face4\": %ld, \"up_face5\": %ld, \"down_face4\": %ld, \"down_face5\": %ld}\n",
         cases, per, wrong, took, fell_back, n_tir, n_refl, n_refr, zero_comp, cos_one, c_zero, c_fmin, fam_n[0], fam_n[1],
         fam_n[2], fam_n[3], fam_n[4], fam_n[5], fam_n[6], fam_n[7], side_face[0][0], side_face[0][1], side_face[1][0],
         side_face[1][1]);
  return wrong ? 1 : 0;
}
