/* Adversarial CPU check of the traversal's closed-form answer about a plane stack (rt_device.h plane_first,
 * scene_compile.cpp plane_stack): before its first visit a ray of the HOP = 4 megakernel instances
 * settles what the stack's own primitives G can return — "none", or the first plane ahead of the origin and beyond
 * tol at the correctly rounded quotient (y_k - o.y) / d.y — and then skips every rect and RectBox leaf; or it
 * declines and runs the leaf tests as before.  Every answer must be what G's leaves return by the reference's rule
 * (hit2 on the leaf box, then the object, t_max = inf, against the running closest) with G walked in either order:
 * the same t bits, primitive and face, or no hit.
 *
 * Everything the answers are judged by comes from tests/ground_hop_check.c, included unchanged (its main renamed);
 * plane_first and the host's record are restated below from the oracle's functions, not taken from the kernel.
 *
 *   ground_first_check <prims file> <draws> [seed [coverage]]
 * Prints one JSON line.  `plane_stack` 0: the stack misses a premise (exit 3).  Rays, one family per draw in turn:
 * origins on, ulps and a little either side of every plane, of Y + tol and of Y + H, and between them; origins and
 * hit points on, ulps off, mx either side of the core's edge and mo either side of the grown extent's; t around
 * t_min and 2 t_min; slopes around the bound and |d.y| around dy_min; upward rays from around tol above Y.
 * Controls, reported and not asserted: the wrong answers among those given only with mx = 0 (and mo = 0), only with
 * tol = 0, only without the H bound.  `coverage`: the family a render produces — camera rays of the headline camera
 * (random_scene's: from (13, 2, 3) at the origin, 20 degrees, 3:2) and rays from the hit points of uniformly drawn
 * rays with refraction, reflection and Lambertian directions — of which plane_first may decline at most 1 % (exit 4
 * otherwise).  Exit 1 when an answer differs.  Test infrastructure (tests/test_ground_first.py); -ffp-contract=off. */
#define main ground_hop_check_main
#include "ground_hop_check.c"
#undef main

static double s_gap, s_tol, s_reach, s_ext, s_sph_top;

/* scene_compile.cpp ground_stack's constants, restated (as in tests/plane_hop_check.c), with the spheres' top */
static void stack_consts(void) {
  double low = INFINITY, ex0 = INFINITY, ex1 = -INFINITY, ez0 = INFINITY, ez1 = -INFINITY, r_min = INFINITY, r_max = 0.0;
  for (int k = 0; k < g_ng; ++k) {
    const prim_c* q = &g_prims[g_g[k]];
    const double* p = q->p;
    if (q->kind == 4) { low = fmin(low, p[1]); ex0 = fmin(ex0, p[0]); ex1 = fmax(ex1, p[3]); ez0 = fmin(ez0, p[2]); ez1 = fmax(ez1, p[5]); }
    else { low = fmin(low, p[4]); ex0 = fmin(ex0, p[0]); ex1 = fmax(ex1, p[1]); ez0 = fmin(ez0, p[2]); ez1 = fmax(ez1, p[3]); }
  }
  double dist = 0.0;
  s_sph_top = y_top;
  for (int i = 0; i < g_n; ++i) {
    const double* p = g_prims[i].p;
    if (g_prims[i].kind != 0 || never_hit(p)) continue;
    r_min = fmin(r_min, p[3]); r_max = fmax(r_max, p[3]);
    s_sph_top = fmax(s_sph_top, p[1] + p[3]);
    const double dx = fmax(fabs(p[0] - ex0), fabs(p[0] - ex1)), dy = fmax(fabs(p[1] - low), fabs(p[1] - y_top));
    const double dz = fmax(fabs(p[2] - ez0), fabs(p[2] - ez1));
    dist = fmax(dist, sqrt(dx * dx + dy * dy + dz * dz));
  }
  const double ratio = 0x1p10, tol = 0x1p-40 * fmax(1.0, fmax(fabs(y_top), fabs(low)));
  const double reach = ((y_top - low) + 2.0 * tol) * (ratio + 1.0);
  const double l2 = (dist + reach) * (dist + reach) + reach * reach + r_max * r_max;
  const double eta = isfinite(r_min) ? 0x1p-38 * l2 / (2.0 * r_min) : 0.0;
  s_gap = 4.0 * eta + 4.0 * tol;
  s_tol = tol;
  s_reach = reach;
  s_ext = fmax(fmax(fabs(ex0), fabs(ex1)), fmax(fabs(ez0), fabs(ez1)));
}

/* scene_compile.cpp plane_stack, restated: the sorted planes, the common core, the grown extent, H and the margins */
typedef struct plane_c {
  double y;
  int prim, face;  /* face 4 / 5 / -1 */
} plane_c;
static plane_c s_pl[8];
static int s_npl;
static double s_core[4], s_outer[4], s_mx, s_mo, s_ymax;  /* the unshrunk core and the ungrown extent: x0 x1 z0 z1 */
static int plane_stack(void) {
  double x0 = -INFINITY, x1 = INFINITY, z0 = -INFINITY, z1 = INFINITY;
  double ux0 = INFINITY, ux1 = -INFINITY, uz0 = INFINITY, uz1 = -INFINITY;
  s_npl = 0;
  for (int k = 0; k < g_ng; ++k) {
    const int i = g_g[k];
    const prim_c* q = &g_prims[i];
    const double* p = q->p;
    const double hx = q->kind == 4 ? p[3] : p[1], hz = q->kind == 4 ? p[5] : p[3];
    x0 = fmax(x0, p[0]); x1 = fmin(x1, hx); z0 = fmax(z0, p[2]); z1 = fmin(z1, hz);
    ux0 = fmin(ux0, p[0]); ux1 = fmax(ux1, hx); uz0 = fmin(uz0, p[2]); uz1 = fmax(uz1, hz);
    if (q->kind == 4) {
      const plane_c lo = {p[1], i, 5}, hi = {p[4], i, 4};
      s_pl[s_npl++] = lo; s_pl[s_npl++] = hi;
    } else {
      const plane_c e = {p[4], i, -1};
      s_pl[s_npl++] = e;
    }
  }
  for (int a = 1; a < s_npl; ++a)
    for (int b = a; b > 0 && s_pl[b].y < s_pl[b - 1].y; --b) { const plane_c e = s_pl[b]; s_pl[b] = s_pl[b - 1]; s_pl[b - 1] = e; }
  for (int a = 1; a < s_npl; ++a)
    if (!(s_pl[a].y - s_pl[a - 1].y > s_gap)) return 0;
  const double mx_hop = 0x1p-44 * (s_ext + s_reach + 1.0);  /* the hop passes' own margin: the plane-stack premise */
  if (!(x0 + mx_hop < x1 - mx_hop && z0 + mx_hop < z1 - mx_hop)) return 0;
  if (gnx > 0 && !(gx0 >= x0 + mx_hop && gx0 + gnx * CELL <= x1 - mx_hop && gz0 >= z0 + mx_hop && gz0 + gnz * CELL <= z1 - mx_hop)) return 0;
  const double height = fmin(0x1p20, fmax(8.0, 2.0 * (s_sph_top - y_top)));
  const double reach_f = s_reach + height * (0x1p10 + 1.0);
  s_mx = 0x1p-44 * (s_ext + reach_f + 1.0);
  s_mo = 0x1p-23 * (s_ext + reach_f + 1.0);
  s_ymax = y_top + height;
  s_core[0] = x0; s_core[1] = x1; s_core[2] = z0; s_core[3] = z1;
  s_outer[0] = ux0; s_outer[1] = ux1; s_outer[2] = uz0; s_outer[3] = uz1;
  return 1;
}

/* rt_device.h plane_first, restated: 0 declined, 1 none, 2 hit.  (`ok`, traverse4's ra_ok: every |d_i| and |d|^2 in
 * [2^-300, 2^300]; its origin limit only makes more rays decline and is far beyond these scenes) */
static int first(const ray_t* r, double mx, double mo, double tol, double y_max, double* t_out, int* prim, int* face) {
  const v3 o = r->o, d = r->d;
  const double ay = fabs(d.y), a = vlen2(d);
  const double lo_d = fmin(fmin(fabs(d.x), ay), fabs(d.z)), hi_d = fmax(fmax(fabs(d.x), ay), fabs(d.z));
  const int ok = lo_d >= 0x1p-300 && hi_d <= 0x1p300 && a >= 0x1p-300 && a <= 0x1p300;
  const double cx0 = s_core[0] + mx, cx1 = s_core[1] - mx, cz0 = s_core[2] + mx, cz1 = s_core[3] - mx;
  if (!(cx0 < cx1 && cz0 < cz1)) return 0;
  if (!(ok && o.y >= y_lo && o.y <= y_max && ay >= dy_min && ay <= 0x1p300 && d.x * d.x + d.z * d.z <= ratio2 * (d.y * d.y) &&
        o.x >= cx0 && o.x <= cx1 && o.z >= cz0 && o.z <= cz1))
    return 0;
  const int up = d.y > 0.0;
  const double hi = o.y + tol, lo = o.y - tol;
  int sel = -1;
  for (int k = 0; k < s_npl; ++k)
    if (up ? (s_pl[k].y > hi && sel < 0) : (s_pl[k].y < lo)) sel = k;
  if (sel < 0) return 1;
  const double t = (s_pl[sel].y - o.y) / d.y;
  if (!(t > 2.0 * T_MIN)) return 0;
  const double hx = o.x + t * d.x, hz = o.z + t * d.z;
  if (!(hx >= cx0 && hx <= cx1 && hz >= cz0 && hz <= cz1)) {
    const int over = o.y > y_hi && (hx < s_outer[0] - mo || hx > s_outer[1] + mo || hz < s_outer[2] - mo || hz > s_outer[3] + mo);
    return over ? 1 : 0;
  }
  *t_out = t; *prim = s_pl[sel].prim; *face = s_pl[sel].face;
  return 2;
}

/* G's leaves by the reference's rule, in G's order or the reverse */
static void g_closest(const ray_t* r, int reverse, double* t, int* best, int* face) {
  *t = INFINITY; *best = -1; *face = -1;
  for (int k = 0; k < g_ng; ++k) leaf_test(g_g[reverse ? g_ng - 1 - k : k], r, t, best, face);
}
static int same(double ta, int pa, int fa, double tb, int pb, int fb) { return pa == pb && fa == fb && !memcmp(&ta, &tb, sizeof ta); }
/* does the answer (kind 1 or 2) differ from G's closest hit under either order? */
static int wrong(const ray_t* r, int kind, double t, int b, int f) {
  int diff = 0;
  for (int rev = 0; rev < 2; ++rev) {
    double te; int be, fe;
    g_closest(r, rev, &te, &be, &fe);
    diff |= kind == 1 ? be >= 0 : !same(t, b, f, te, be, fe);
  }
  return diff;
}
static v3 unit_vector(void) {
  for (;;) {
    const v3 p = V(range(-1.0, 1.0), range(-1.0, 1.0), range(-1.0, 1.0));
    if (vlen2(p) <= 1.0 && vlen2(p) > 1e-12) return vunit(p);
  }
}
static double around(double e, double m) {  /* a value on, ulps off, m off, ulps off that, or a little off e */
  const int k = (int)(next_u64() % 6);
  const double s = unif() < 0.5 ? -1.0 : 1.0;
  return k == 0 ? e : k == 1 ? ulps(e, (int)(next_u64() % 9) - 4) : k == 2 ? e + s * m : k == 3 ? ulps(e + s * m, (int)(next_u64() % 9) - 4)
         : k == 4 ? e + s * m * range(0.5, 2.0) : e + s * logu(1e-16, 1e-3);
}

/* the closest hit over the whole scene with its geometric normal against the ray (the coverage family's first hits) */
static int first_hit(const ray_t* q, v3* p, v3* n, int* diel) {
  double te; int be, fe;
  exhaustive(q, 1, &te, &be, &fe);
  if (be < 0) return 0;
  *p = ray_at(q, te);
  const prim_c* s = &g_prims[be];
  v3 out;
  if (s->kind == 0) out = vscale(V(p->x - s->p[0], p->y - s->p[1], p->z - s->p[2]), 1.0 / s->p[3]);
  else if (fe >= 0 && fe < 2) out = V(0.0, 0.0, 1.0);
  else if (fe >= 2 && fe < 4) out = V(1.0, 0.0, 0.0);
  else out = V(0.0, 1.0, 0.0);
  *n = vdot(q->d, out) < 0.0 ? out : vscale(out, -1.0);
  *diel = s->diel;
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  const long n = atol(argv[2]);
  if (argc > 3) s_state = (s_state + strtoull(argv[3], NULL, 0) * 0xD1B54A32D192ED03ull) | 1ull;
  const int coverage = argc > 4 && !strcmp(argv[4], "coverage");
  int cap = 1024;
  g_prims = malloc(cap * sizeof *g_prims);
  char w[8][64];
  while (fscanf(f, "%63s %63s %63s %63s %63s %63s %63s %63s", w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]) == 8) {
    if (g_n == cap) g_prims = realloc(g_prims, (cap *= 2) * sizeof *g_prims);
    g_prims[g_n].kind = atoi(w[0]);
    g_prims[g_n].diel = atoi(w[1]);
    for (int k = 0; k < 6; ++k) g_prims[g_n].p[k] = strtod(w[2 + k], NULL);
    ++g_n;
  }
  fclose(f);
  build_reference();
  if (!ground_stack()) { printf("{\"ground_stack\": 0, \"plane_stack\": 0}\n"); return 3; }
  stack_consts();
  if (!plane_stack()) { printf("{\"ground_stack\": 1, \"plane_stack\": 0}\n"); return 3; }
  /* the heights an origin is drawn around: every plane, Y + tol and Y + H */
  double lv[10];
  int n_lv = 0;
  for (int k = 0; k < s_npl; ++k) lv[n_lv++] = s_pl[k].y;
  lv[n_lv++] = y_hi;
  lv[n_lv++] = s_ymax;
  const double cx0 = s_core[0] + s_mx, cx1 = s_core[1] - s_mx, cz0 = s_core[2] + s_mx, cz1 = s_core[3] - s_mx;
  long hits = 0, nones = 0, declined = 0, over_nones = 0, up_nones = 0, ans_wrong = 0, edge_answers = 0, above_hits = 0;
  long mx0_answers = 0, mx0_wrong = 0, tol0_changed = 0, tol0_wrong = 0, noh_answers = 0, noh_wrong = 0;
  for (long it = 0; it < n; ++it) {
    const int fam = (int)(it % 5);
    ray_t r;
    v3 a, b;
    /* origin height: on, ulps around, a little off one of the levels, or between two of them */
    const double from = lv[next_u64() % (uint64_t)n_lv];
    const int hm = (int)(next_u64() % 5);
    a.y = hm == 0 ? from : hm == 1 ? ulps(from, (int)(next_u64() % 9) - 4) : hm == 2 ? from + range(-4.0, 4.0) * s_tol
          : hm == 3 ? range(y_lo, s_ymax) : from + (unif() < 0.5 ? -1.0 : 1.0) * logu(1e-15, 1e-2);
    a.x = range(cx0, cx1); a.z = range(cz0, cz1);
    /* aimed at a point of a plane of G (or, one time in four, up or down freely) */
    const double to = s_pl[next_u64() % (uint64_t)s_npl].y;
    b.y = to;
    double run = fabs(b.y - a.y) * logu(1e-3, 1e3);
    if (fam == 3) run = fabs(b.y - a.y) * 0x1p10 * (1.0 + range(-1e-6, 1e-6));  /* the slope bound */
    const double an = range(0.0, 6.283185307179586);
    b.x = a.x + run * cos(an); b.z = a.z + run * sin(an);
    if (fam == 1) {
      /* the origin or the hit point around an edge of the core, or the hit point around the grown extent's */
      const int em = (int)(next_u64() % 4), sx = (int)(next_u64() & 1), sz = (int)(next_u64() & 1);
      const double ex = s_core[sx] + (sx ? -s_mx : s_mx), ez = s_core[2 + sz] + (sz ? -s_mx : s_mx);
      const double ox = s_outer[sx] + (sx ? s_mo : -s_mo), oz = s_outer[2 + sz] + (sz ? s_mo : -s_mo);
      if (em == 0) { const double s = around(ex, s_mx) - b.x; a.x += s; b.x += s; if (next_u64() & 1) { const double q = around(ez, s_mx) - b.z; a.z += q; b.z += q; } }
      else if (em == 1) { const double s = around(ex, s_mx) - a.x; a.x += s; b.x += s; if (next_u64() & 1) { const double q = around(ez, s_mx) - a.z; a.z += q; b.z += q; } }
      else if (em == 2) { b.x = around(ox, s_mo); if (next_u64() & 1) b.z = around(oz, s_mo); }
      else { b.z = around(oz, s_mo); b.x = (next_u64() & 1) ? around(ex, s_mx) : b.x; }
    }
    r.o = a;
    r.d = V(b.x - a.x, b.y - a.y, b.z - a.z);
    if ((next_u64() & 3) == 0) {  /* free directions: mostly steep, some shallow */
      const double sy = (unif() < 0.5 ? -1.0 : 1.0) * (unif() < 0.5 ? logu(1e-9, 1.0) : range(0.0, 1.0)), sxz = sqrt(fmax(0.0, 1.0 - sy * sy));
      r.d = V(sxz * cos(an), sy, sxz * sin(an));
    }
    r.d = vscale(r.d, (next_u64() & 3) == 0 ? logu(1e-3, 1e3) : range(0.5, 2.0) / fmax(vlen(r.d), 1e-300));
    if (fam == 3 && (next_u64() & 1)) {  /* |d.y| around dy_min */
      const double s = dy_min * (1.0 + range(-1e-6, 1e-6)) / fmax(fabs(r.d.y), 1e-300);
      r.d = vscale(r.d, s);
    }
    if (fam == 2) {  /* t around t_min and 2 t_min */
      const double k = (next_u64() & 1) ? 1.0 : 2.0;
      r.o.y = to - r.d.y * T_MIN * k * (1.0 + range(-1e-9, 1e-9) * (double)(next_u64() % 3));
      if (next_u64() & 1) r.o.y = ulps(to - r.d.y * T_MIN * k, (int)(next_u64() % 9) - 4);
    }
    if (fam == 4) {  /* upward from around tol above Y (and, as often, above the other levels) */
      r.d.y = fabs(r.d.y);
      if (next_u64() & 1) r.o.y = (next_u64() & 1) ? ulps(y_hi, (int)(next_u64() % 9) - 4) : y_top + s_tol * range(0.0, 2.0);
    }
    double t = 0.0; int pb = -1, fc = -1;
    const int kind = first(&r, s_mx, s_mo, s_tol, s_ymax, &t, &pb, &fc);
    if (kind) {
      hits += kind == 2; nones += kind == 1; edge_answers += fam == 1;
      above_hits += kind == 2 && r.o.y > y_hi;
      up_nones += kind == 1 && r.d.y > 0.0;
      over_nones += kind == 1 && r.d.y < 0.0 && r.o.y > y_hi;
      const int wr = wrong(&r, kind, t, pb, fc);
      ans_wrong += wr;
      if (wr && ans_wrong <= 8) {
        double te; int be, fe;
        g_closest(&r, 0, &te, &be, &fe);
        fprintf(stderr, "answer differs: o %a %a %a d %a %a %a: plane_first kind %d prim %d face %d t %a, G's leaves prim %d face %d t %a\n",
                r.o.x, r.o.y, r.o.z, r.d.x, r.d.y, r.d.z, kind, pb, fc, t, be, fe, te);
      }
    } else {
      ++declined;
    }
    /* controls: answers given only with a premise off */
    double tc; int bc, fcc;
    const int k0 = first(&r, 0.0, 0.0, s_tol, s_ymax, &tc, &bc, &fcc);
    if (k0 && !kind) { ++mx0_answers; mx0_wrong += wrong(&r, k0, tc, bc, fcc); }
    const int kt = first(&r, s_mx, s_mo, 0.0, s_ymax, &tc, &bc, &fcc);
    if (kt != kind || (kt == 2 && !same(t, pb, fc, tc, bc, fcc))) { ++tol0_changed; if (kt) tol0_wrong += wrong(&r, kt, tc, bc, fcc); }
    const int kh = first(&r, s_mx, s_mo, s_tol, INFINITY, &tc, &bc, &fcc);
    if (kh && !kind) { ++noh_answers; noh_wrong += wrong(&r, kh, tc, bc, fcc); }
  }
  /* the coverage family: what a render traces */
  long cov_rays = 0, cov_camera = 0, cov_declined = 0, cov_camera_declined = 0, cov_wrong = 0, cov_none = 0;
  if (coverage) {
    /* the headline camera (scenes.rs default_camera on a 3:2 frame), pinhole */
    const v3 from = V(13.0, 2.0, 3.0), wv = vunit(from), uv = vunit(V(wv.z, 0.0, -wv.x));  /* vup x w */
    const v3 vv = V(wv.y * uv.z - wv.z * uv.y, wv.z * uv.x - wv.x * uv.z, wv.x * uv.y - wv.y * uv.x);
    const double hh = tan(20.0 * 3.14159265358979323846 / 360.0), hw = 1.5 * hh;
    while (cov_rays < n / 3) {
      ray_t r;
      const int cam = cov_rays % 3 == 0;
      if (cam) {
        const double s = range(-1.0, 1.0) * hw, u = range(-1.0, 1.0) * hh;
        r.o = from;
        r.d = vscale(V(s * uv.x + u * vv.x - wv.x, s * uv.y + u * vv.y - wv.y, s * uv.z + u * vv.z - wv.z), 10.0);
      } else {
        ray_t q;
        q.o = V(range(-14.0, 14.0), y_top + range(0.0, 3.0), range(-14.0, 14.0));
        q.d = unit_vector();
        v3 p, nrm;
        int diel;
        if (!first_hit(&q, &p, &nrm, &diel)) continue;
        r.o = p;
        const v3 ud = vunit(q.d);
        if (diel) {
          const int front = vdot(q.d, nrm) < 0.0;  /* (nrm is against the ray: always; the ratio by a coin instead) */
          const double ratio = (front && (next_u64() & 1)) ? 1.0 / 1.5 : 1.5;
          const double ct = fmin(vdot(vscale(ud, -1.0), nrm), 1.0), st = sqrt(1.0 - ct * ct);
          r.d = ratio * st > 1.0 ? reflect(ud, nrm) : refract(ud, nrm, ratio);
        } else if (next_u64() & 1) {
          r.d = vadd(nrm, unit_vector());
        } else {
          r.d = reflect(ud, nrm);
        }
      }
      ++cov_rays;
      cov_camera += cam;
      double t = 0.0; int pb = -1, fc = -1;
      const int kind = first(&r, s_mx, s_mo, s_tol, s_ymax, &t, &pb, &fc);
      if (!kind) { ++cov_declined; cov_camera_declined += cam; }
      else { cov_none += kind == 1; cov_wrong += wrong(&r, kind, t, pb, fc); }
    }
  }
  /* the record as scene_compile.cpp packs it, without the primitive numbers (the device's are the tree's leaf ranks) */
  printf("{\"plane_y\": [");
  for (int k = 0; k < s_npl; ++k) printf("%s\"%a\"", k ? ", " : "", s_pl[k].y);
  printf("], \"core_first\": [\"%a\", \"%a\", \"%a\", \"%a\"], \"outer\": [\"%a\", \"%a\", \"%a\", \"%a\"], \"y_max\": \"%a\", ", cx0, cx1, cz0, cz1,
         s_outer[0] - s_mo, s_outer[1] + s_mo, s_outer[2] - s_mo, s_outer[3] + s_mo, s_ymax);
  printf("\"ground_stack\": 1, \"plane_stack\": 1, \"planes\": %d, \"draws\": %ld, \"hits\": %ld, \"hits_from_above\": %ld, \"nones\": %ld, "
         "\"nones_upward\": %ld, \"nones_over_edge\": %ld, \"declined\": %ld, \"edge_answers\": %ld, \"wrong\": %ld, "
         "\"mx0_extra_answers\": %ld, \"mx0_wrong\": %ld, \"tol0_changed\": %ld, \"tol0_wrong\": %ld, \"no_h_extra_answers\": %ld, "
         "\"no_h_wrong\": %ld, \"coverage_rays\": %ld, \"coverage_camera\": %ld, \"coverage_declined\": %ld, "
         "\"coverage_camera_declined\": %ld, \"coverage_none\": %ld, \"coverage_wrong\": %ld, \"mx\": %.17g, \"mo\": %.17g, \"tol\": %.17g}\n",
         s_npl, n, hits, above_hits, nones, up_nones, over_nones, declined, edge_answers, ans_wrong, mx0_answers, mx0_wrong, tol0_changed,
         tol0_wrong, noh_answers, noh_wrong, cov_rays, cov_camera, cov_declined, cov_camera_declined, cov_none, cov_wrong, s_mx, s_mo, s_tol);
  if (ans_wrong || cov_wrong) return 1;
  if (coverage && !(cov_rays > 0 && cov_declined * 100 <= cov_rays)) return 4;
  return 0;
}
