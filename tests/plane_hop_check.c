/* Adversarial CPU check of the plane-stack hop decision (rt_device.h plane_hop_t, scene_compile.cpp plane_stack;
 * DESIGN.md §3.1): for a ray that starts inside a stack of horizontal slabs, steep enough to meet only y planes,
 * the next hit is the first plane of the sorted plane list beyond the one it stands on, at the correctly rounded
 * quotient (y_k - o.y) / d.y — answered only when origin and hit point lie inside the primitives' common xz core
 * shrunk by mx, t > 2 t_min, and an exit through the top plane finds a free guard cell.  Every answered ray must
 * carry the (t bits, primitive, face, kind) of the general decision (ground_hop_t<true>, restated as in
 * tests/down_hop_check.c) and of the exhaustive closest hit with G tested first and last, and of the reference's own
 * walk of its own tree.
 *
 * Everything the decisions are judged by comes from tests/ground_hop_check.c, included unchanged (its main renamed);
 * the general decision's extension to found hits is restated from tests/down_hop_check.c; the fast decision and the
 * host's plane_stack are restated below from the oracle's functions, not taken from the kernel.
 *
 *   plane_hop_check <prims file> <draws> [seed [coverage]]
 * Prints one JSON line.  `plane_stack` 0: the stack misses a premise (exit 3).  Rays: down_hop_check's draws (origins
 * on, between and ulps either side of every plane, slopes around the bound, |d.y| around dy_min, exits aimed at
 * contact points), and, one draw in three, the fast path's own edges: origins and hit points on, ulps off and mx
 * either side of the core's edge, t around t_min and 2 t_min.  Controls: how many answers would differ from the
 * exhaustive hit with mx = 0, and how many answers change with the standing-plane rule off (tol = 0); reported, not
 * asserted.  `coverage`: a non-adversarial family as well — origins are the hit points of uniformly drawn rays on
 * the stack, directions come from the refraction and Lambertian expressions — on which the fast decision may
 * decline at most 1 % of the rays the general decision answers (exit 4 otherwise).  Exit 1 when an answered ray
 * differs.  Test infrastructure (tests/test_plane_hop.py); -ffp-contract=off. */
#define main ground_hop_check_main
#include "ground_hop_check.c"
#undef main

static double y_down, s_gap, s_tol, s_reach, s_ext;  /* Y - gap, gap, tol, reach, the largest |x|, |z| of G */

/* scene_compile.cpp ground_stack's constants, restated with ground_hop_check.c ground_stack's names */
static void stack_consts(void) {
  double low = INFINITY, ex0 = INFINITY, ex1 = -INFINITY, ez0 = INFINITY, ez1 = -INFINITY, r_min = INFINITY, r_max = 0.0;
  for (int k = 0; k < g_ng; ++k) {
    const prim_c* q = &g_prims[g_g[k]];
    const double* p = q->p;
    if (q->kind == 4) { low = fmin(low, p[1]); ex0 = fmin(ex0, p[0]); ex1 = fmax(ex1, p[3]); ez0 = fmin(ez0, p[2]); ez1 = fmax(ez1, p[5]); }
    else { low = fmin(low, p[4]); ex0 = fmin(ex0, p[0]); ex1 = fmax(ex1, p[1]); ez0 = fmin(ez0, p[2]); ez1 = fmax(ez1, p[3]); }
  }
  double dist = 0.0;
  for (int i = 0; i < g_n; ++i) {
    const double* p = g_prims[i].p;
    if (g_prims[i].kind != 0 || never_hit(p)) continue;
    r_min = fmin(r_min, p[3]); r_max = fmax(r_max, p[3]);
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

/* The general decision (tests/down_hop_check.c decide, restated): 0 refused, 1 served, 2 found. */
static int decide(const ray_t* r, double* t_best, int* best, int* face) {
  int og, os, ot;
  const int sv = serve(r, t_best, best, face, &og, &os, &ot);  /* (also leaves G's closest hit in the outputs) */
  if (sv) return 1;
  if (*best < 0 || g_prims[*best].diel) return 0;
  int tie = 0, b = -1, f = -1;
  double tb = INFINITY;
  for (int k = 0; k < g_ng; ++k) {
    const int i = g_g[k];
    const prim_c* q = &g_prims[i];
    const aabb_t lb = leaf_box_of(q);
    if (!aabb_hit2(lb, r, T_MIN, tb)) {
      if (k < g_nbox && b >= 0 && near_entry(slab_entry(lb, r, T_MIN), tb)) tie = 1;
      continue;
    }
    double t;
    int fc = -1;
    hit_t h;
    if (k < g_nbox) { fc = box_hit_face(q->p, r, T_MIN, tb, &t); if (fc < 0) continue; }
    else { if (!rect_hit(0, 2, q->p, r, T_MIN, tb, &h)) continue; t = h.t; }
    if (t == tb && b >= 0) {
      if (tie) continue;
      if (!(g_rank[i] < g_rank[b]) && aabb_hit2(leaf_box_of(&g_prims[b]), r, T_MIN, t)) continue;
    }
    tb = t; b = i; f = fc; tie = 0;
  }
  if (tie || (f >= 0 && f < 4) || !(tb > T_MIN)) return 0;
  const double ay = fabs(r->d.y);
  if (!(r->o.y >= y_lo && r->o.y <= y_hi && ay >= dy_min && ay <= 0x1p300)) return 0;
  if (!(r->d.x * r->d.x + r->d.z * r->d.z <= ratio2 * (r->d.y * r->d.y))) return 0;
  const double y = g_prims[b].kind == 3 ? g_prims[b].p[4] + 0.0001 : (f == 4 ? g_prims[b].p[4] : g_prims[b].p[1]);
  return y <= y_down ? 2 : 0;
}

/* scene_compile.cpp plane_stack, restated: the sorted plane list, the common core and its margin */
typedef struct plane_c {
  double y;
  int prim, face, kind, top;  /* face 4 / 5 / -1; kind 0 never answered, 1 served, 2 found */
} plane_c;
static plane_c s_pl[8];
static int s_npl;
static double s_core[4], s_mx;  /* the unshrunk core x0 x1 z0 z1 */
static int plane_stack(void) {
  double x0 = -INFINITY, x1 = INFINITY, z0 = -INFINITY, z1 = INFINITY;
  s_npl = 0;
  for (int k = 0; k < g_ng; ++k) {
    const int i = g_g[k];
    const prim_c* q = &g_prims[i];
    const double* p = q->p;
    if (q->kind == 4) {
      x0 = fmax(x0, p[0]); x1 = fmin(x1, p[3]); z0 = fmax(z0, p[2]); z1 = fmin(z1, p[5]);
      for (int s = 0; s < 2; ++s) {
        const double y = s ? p[4] : p[1];
        const plane_c e = {y, i, s ? 4 : 5, q->diel ? 1 : (y <= y_down ? 2 : 0), y == y_top};
        s_pl[s_npl++] = e;
      }
    } else {
      x0 = fmax(x0, p[0]); x1 = fmin(x1, p[1]); z0 = fmax(z0, p[2]); z1 = fmin(z1, p[3]);
      const plane_c e = {p[4], i, -1, (!q->diel && p[4] + 0.0001 <= y_down) ? 2 : 0, 0};
      s_pl[s_npl++] = e;
    }
  }
  for (int a = 1; a < s_npl; ++a)
    for (int b = a; b > 0 && s_pl[b].y < s_pl[b - 1].y; --b) { const plane_c e = s_pl[b]; s_pl[b] = s_pl[b - 1]; s_pl[b - 1] = e; }
  for (int a = 1; a < s_npl; ++a)
    if (!(s_pl[a].y - s_pl[a - 1].y > s_gap)) return 0;
  s_mx = 0x1p-44 * (s_ext + s_reach + 1.0);
  s_core[0] = x0; s_core[1] = x1; s_core[2] = z0; s_core[3] = z1;
  if (!(x0 + s_mx < x1 - s_mx && z0 + s_mx < z1 - s_mx)) return 0;
  if (gnx > 0 && !(gx0 >= x0 + s_mx && gx0 + gnx * CELL <= x1 - s_mx && gz0 >= z0 + s_mx && gz0 + gnz * CELL <= z1 - s_mx)) return 0;
  return 1;
}

/* rt_device.h plane_hop_t<true>, restated: 0 declined, 1 served, 2 found */
static int fast(const ray_t* r, double mx, double tol, double* t_out, int* prim, int* face) {
  const v3 o = r->o, d = r->d;
  const double ay = fabs(d.y);
  const double cx0 = s_core[0] + mx, cx1 = s_core[1] - mx, cz0 = s_core[2] + mx, cz1 = s_core[3] - mx;
  if (!(o.y >= y_lo && o.y <= y_hi && ay >= dy_min && ay <= 0x1p300 && d.x * d.x + d.z * d.z <= ratio2 * (d.y * d.y))) return 0;
  if (!(o.x >= cx0 && o.x <= cx1 && o.z >= cz0 && o.z <= cz1)) return 0;
  const int up = d.y > 0.0;
  const double hi = o.y + tol, lo = o.y - tol;
  int sel = -1;
  for (int k = 0; k < s_npl; ++k) {
    if (up ? (s_pl[k].y > hi && sel < 0) : (s_pl[k].y < lo)) sel = k;
  }
  if (sel < 0 || s_pl[sel].kind == 0) return 0;
  const double t = (s_pl[sel].y - o.y) / d.y;
  if (!(t > 2.0 * T_MIN)) return 0;
  const double hx = o.x + t * d.x, hz = o.z + t * d.z;
  if (!(hx >= cx0 && hx <= cx1 && hz >= cz0 && hz <= cz1)) return 0;
  if (s_pl[sel].top && s_pl[sel].kind == 1) {
    const int ix = cell_of(hx, gx0, gnx), iz = cell_of(hz, gz0, gnz);
    if (ix >= 0 && iz >= 0) {
      const size_t c = (size_t)iz * gnx + ix;
      if ((g_bits[c >> 5] >> (c & 31)) & 1u) return 0;
    }
  }
  *t_out = t; *prim = s_pl[sel].prim; *face = s_pl[sel].face;
  return s_pl[sel].kind;
}

static int same(double ta, int pa, int fa, double tb, int pb, int fb) { return pa == pb && fa == fb && !memcmp(&ta, &tb, sizeof ta); }
/* does the answer (kind > 0) differ from the exhaustive closest hit under either order, or from the reference's walk? */
static int wrong(const ray_t* r, double t, int b, int f) {
  double te; int be, fe, diff = 0;
  for (int gf = 0; gf < 2; ++gf) {
    exhaustive(r, gf, &te, &be, &fe);
    diff |= !same(t, b, f, te, be, fe);
  }
  reference(r, &te, &be, &fe);
  return diff | !same(t, b, f, te, be, fe);
}
static v3 unit_vector(void) {
  for (;;) {
    const v3 p = V(range(-1.0, 1.0), range(-1.0, 1.0), range(-1.0, 1.0));
    if (vlen2(p) <= 1.0 && vlen2(p) > 1e-12) return vunit(p);
  }
}
static double edge_of(double e, double mx) {  /* a coordinate on, ulps off, mx off or a little off an edge value */
  const int m = (int)(next_u64() % 6);
  const double s = unif() < 0.5 ? -1.0 : 1.0;
  return m == 0 ? e : m == 1 ? ulps(e, (int)(next_u64() % 9) - 4) : m == 2 ? e + s * mx : m == 3 ? ulps(e + s * mx, (int)(next_u64() % 9) - 4)
         : m == 4 ? e + s * mx * range(0.5, 2.0) : e + s * logu(1e-16, 1e-3);
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
  y_down = y_top - s_gap;
  if (!plane_stack()) { printf("{\"ground_stack\": 1, \"plane_stack\": 0}\n"); return 3; }
  int* sph = malloc(g_n * sizeof *sph), n_sph = 0;
  double pl[8], xlo = INFINITY, xhi = -INFINITY, zlo = INFINITY, zhi = -INFINITY;
  int n_pl = 0;
  for (int i = 0; i < g_n; ++i) {
    const double* p = g_prims[i].p;
    if (g_prims[i].kind == 0) { if (!never_hit(p)) sph[n_sph++] = i; continue; }
    if (g_prims[i].kind == 4) { pl[n_pl++] = p[1]; pl[n_pl++] = p[4]; xlo = fmin(xlo, p[0]); xhi = fmax(xhi, p[3]); zlo = fmin(zlo, p[2]); zhi = fmax(zhi, p[5]); }
    else { pl[n_pl++] = p[4]; xlo = fmin(xlo, p[0]); xhi = fmax(xhi, p[1]); zlo = fmin(zlo, p[2]); zhi = fmax(zhi, p[3]); }
  }
  long served = 0, found = 0, ans_wrong = 0, ans_not_general = 0, general = 0, declined = 0, edge_answers = 0;
  long mx0_answers = 0, mx0_wrong = 0, stand_changed = 0, stand_wrong = 0;
  for (long it = 0; it < n; ++it) {
    ray_t r;
    if (it % 3 == 2) {
      /* the fast path's own edges: from a plane of G (on it or ulps off) to another, the origin or the hit point on,
       * ulps off or mx off an edge of the core; one time in three t around t_min or 2 t_min instead */
      const double from = pl[next_u64() % (uint64_t)n_pl], to = pl[next_u64() % (uint64_t)n_pl];
      const int em = (int)(next_u64() % 4);
      v3 a, b;
      a.y = (next_u64() & 1) ? from : ulps(from, (int)(next_u64() % 9) - 4);
      b.y = to;
      a.x = range(s_core[0], s_core[1]); a.z = range(s_core[2], s_core[3]);
      const double run = fabs(b.y - a.y) * (unif() < 0.3 ? 0x1p10 * (1.0 + range(-1e-6, 1e-6)) : logu(1e-3, 1e3)), an = range(0.0, 6.283185307179586);
      b.x = a.x + run * cos(an); b.z = a.z + run * sin(an);
      const double ex = s_core[next_u64() & 1], ez = s_core[2 + (next_u64() & 1)];
      if (em == 0) { const double sx = edge_of(ex, s_mx) - b.x; a.x += sx; b.x += sx; if (next_u64() & 1) { const double sz = edge_of(ez, s_mx) - b.z; a.z += sz; b.z += sz; } }
      else if (em == 1) { const double sz = edge_of(ez, s_mx) - b.z; a.z += sz; b.z += sz; }
      else if (em == 2) { const double sx = edge_of(ex, s_mx) - a.x; a.x += sx; b.x += sx; if (next_u64() & 1) { const double sz = edge_of(ez, s_mx) - a.z; a.z += sz; b.z += sz; } }
      r.o = a;
      r.d = V(b.x - a.x, b.y - a.y, b.z - a.z);
      r.d = vscale(r.d, (next_u64() & 3) == 0 ? logu(1e-3, 1e3) : range(0.5, 2.0) / fmax(vlen(r.d), 1e-300));
      if (em == 3) {
        const double k = (next_u64() & 1) ? 1.0 : 2.0;
        r.o.y = to - r.d.y * T_MIN * k * (1.0 + range(-1e-9, 1e-9) * (double)(next_u64() % 3));
        if (next_u64() & 1) r.o.y = ulps(to - r.d.y * T_MIN * k, (int)(next_u64() % 9) - 4);
      }
    } else {
      /* tests/down_hop_check.c's draws */
      int mode = (int)(next_u64() % 8);
      if (!n_sph && mode != 0 && mode != 2 && mode != 7) {
        static const int other[3] = {0, 2, 7};
        mode = other[next_u64() % 3];
      }
      const double* sp = n_sph ? g_prims[sph[next_u64() % (uint64_t)n_sph]].p : NULL;
      const double plane = pl[next_u64() % (uint64_t)n_pl];
      const int hm = (int)(next_u64() % 6);
      r.o.y = hm == 0 ? plane : hm == 1 ? ulps(plane, (int)(next_u64() % 9) - 4) : hm == 2 ? plane + range(-1e-12, 1e-12)
              : hm == 3 ? range(y_lo, y_hi) : hm == 4 ? plane + (unif() < 0.5 ? -1.0 : 1.0) * logu(1e-15, 1e-3) : plane;
      if (mode == 0 || (mode == 7 && !sp)) { r.o.x = range(xlo, xhi); r.o.z = range(zlo, zhi); }
      else if (mode == 1) { r.o.x = sp[0]; r.o.z = sp[2]; if (unif() < 0.5) { r.o.x = ulps(r.o.x, (int)(next_u64() % 5) - 2); r.o.z += range(-1e-9, 1e-9); } }
      else if (mode == 2) { const double e = logu(1e-12, 1e-2); r.o.x = (unif() < 0.5 ? xlo : xhi) + range(-e, e); r.o.z = (unif() < 0.5 ? zlo : zhi) + range(-e, e); if (unif() < 0.5) r.o.z = range(zlo, zhi); }
      else { const double rho = mode == 3 ? logu(1e-6, 0.5) : logu(1e-3, 8.0), a = range(0.0, 6.283185307179586); r.o.x = sp[0] + rho * cos(a); r.o.z = sp[2] + rho * sin(a); }
      if (mode >= 3 && mode <= 6) {
        const double off = logu(1e-17, 1e-1), a = range(0.0, 6.283185307179586);
        const int vm = (int)(next_u64() % 4);
        const double tx = sp[0] + off * cos(a), tz = sp[2] + off * sin(a);
        const double ty = vm == 0 ? y_top : vm == 1 ? ulps(y_top, (int)(next_u64() % 5) - 2) : vm == 2 ? y_top + logu(1e-17, 1e-6) : y_top - logu(1e-17, 1e-6);
        r.d = V(tx - r.o.x, ty - r.o.y, tz - r.o.z);
        if (mode == 6) r.d.y = (unif() < 0.5 ? -1.0 : 1.0) * logu(1e-9, 1e-2) * sqrt(r.d.x * r.d.x + r.d.z * r.d.z);
      } else {
        const double a = range(0.0, 6.283185307179586), sy = (unif() < 0.5 ? -1.0 : 1.0) * (unif() < 0.5 ? logu(1e-9, 1.0) : range(0.0, 1.0));
        const double sxz = sqrt(fmax(0.0, 1.0 - sy * sy));
        r.d = V(sxz * cos(a), sy, sxz * sin(a));
      }
      if ((next_u64() & 3) == 0 && n_pl > 1) {
        const double from = pl[next_u64() % (uint64_t)n_pl], to = pl[next_u64() % (uint64_t)n_pl];
        r.o.y = ulps(from, (int)(next_u64() % 9) - 4);
        const double a = range(0.0, 6.283185307179586), dy = to - r.o.y;
        const int km = (int)(next_u64() % 4);
        const double run = km == 0 ? fabs(dy) * 0x1p10 * (1.0 + range(-1e-6, 1e-6)) : km == 1 ? fabs(dy) * logu(1e-3, 1e5) : range(0.0, 2.0) * fabs(dy);
        r.d = V(run * cos(a), dy, run * sin(a));
        if (km == 3) { const double s = dy_min * (1.0 + range(-1e-6, 1e-6)) / fmax(fabs(dy), 1e-300); r.d = vscale(r.d, s); }
      }
      const double sc = (next_u64() & 3) == 0 ? logu(1e-3, 1e3) : range(0.5, 2.0);
      r.d = vscale(r.d, sc);
      if (mode == 7) {
        const double target = pl[next_u64() % (uint64_t)n_pl];
        r.o.y = target - r.d.y * T_MIN * ((next_u64() & 1) ? 1.0 : 2.0) * (1.0 + range(-1e-9, 1e-9) * (double)(next_u64() % 3));
      }
    }
    double t = 0.0, tg = 0.0; int b = -1, fc = -1, bg = -1, fg = -1;
    const int kind = fast(&r, s_mx, s_tol, &t, &b, &fc);
    const int kg = decide(&r, &tg, &bg, &fg);
    general += kg != 0;
    if (kind) {
      served += kind == 1; found += kind == 2; edge_answers += it % 3 == 2;
      const int wr = wrong(&r, t, b, fc), ng = !(kg == kind && same(t, b, fc, tg, bg, fg));
      ans_wrong += wr; ans_not_general += ng;
      if ((wr || ng) && ans_wrong + ans_not_general <= 8)
        fprintf(stderr, "answered ray differs: o %a %a %a d %a %a %a: fast kind %d prim %d face %d t %a, general kind %d prim %d face %d t %a, wrong %d\n",
                r.o.x, r.o.y, r.o.z, r.d.x, r.d.y, r.d.z, kind, b, fc, t, kg, bg, fg, tg, wr);
    } else if (kg) {
      ++declined;
    }
    /* controls */
    double tc; int bc, fcc;
    const int k0 = fast(&r, 0.0, s_tol, &tc, &bc, &fcc);
    if (k0 && !kind) { ++mx0_answers; mx0_wrong += wrong(&r, tc, bc, fcc); }
    const int ks = fast(&r, s_mx, 0.0, &tc, &bc, &fcc);
    if (ks != kind || (ks && !same(t, b, fc, tc, bc, fcc))) { ++stand_changed; if (ks) stand_wrong += wrong(&r, tc, bc, fcc); }
  }
  /* the coverage family */
  long cov_general = 0, cov_declined = 0, cov_wrong = 0, cov_rays = 0;
  if (coverage) {
    const double ix0 = s_core[0] + 1.0, ix1 = s_core[1] - 1.0, iz0 = s_core[2] + 1.0, iz1 = s_core[3] - 1.0;  /* interior rays */
    while (cov_rays < n / 3) {
      ray_t q;
      q.o = V(range(ix0, ix1), unif() < 0.5 ? y_top + range(0.0, 2.0) : range(y_lo, y_hi), range(iz0, iz1));
      q.d = unit_vector();
      double te; int be, fe;
      exhaustive(&q, 1, &te, &be, &fe);
      if (be < 0 || g_prims[be].kind == 0 || (fe >= 0 && fe < 4)) continue;
      const v3 p = ray_at(&q, te);
      const v3 nrm = V(0.0, q.d.y < 0.0 ? 1.0 : -1.0, 0.0);  /* against the ray */
      ray_t r;
      r.o = p;
      if (g_prims[be].diel) {
        const v3 ud = vunit(q.d);
        const int front = fe == 4 ? q.d.y < 0.0 : q.d.y > 0.0;  /* the outward normal of face 4 is +y, of face 5 -y */
        const double ratio = front ? 1.0 / 1.5 : 1.5;
        const double ct = fmin(vdot(vscale(ud, -1.0), nrm), 1.0), st = sqrt(1.0 - ct * ct);
        r.d = ratio * st > 1.0 ? reflect(ud, nrm) : refract(ud, nrm, ratio);
      } else {
        r.d = vadd(nrm, unit_vector());
      }
      ++cov_rays;
      double t = 0.0, tg = 0.0; int b = -1, fc = -1, bg = -1, fg = -1;
      const int kg = decide(&r, &tg, &bg, &fg);
      if (!kg) continue;
      ++cov_general;
      const int kind = fast(&r, s_mx, s_tol, &t, &b, &fc);
      if (!kind) ++cov_declined;
      else cov_wrong += !(kg == kind && same(t, b, fc, tg, bg, fg)) || wrong(&r, t, b, fc);
    }
  }
  /* the record as scene_compile.cpp packs it, without the primitive numbers (the device's are the tree's leaf ranks) */
  printf("{\"plane_y\": [");
  for (int k = 0; k < s_npl; ++k) printf("%s\"%a\"", k ? ", " : "", s_pl[k].y);
  printf("], \"plane_code\": [");
  for (int k = 0; k < s_npl; ++k)
    printf("%s%d", k ? ", " : "", (s_pl[k].top ? 16 : 0) | s_pl[k].kind << 2 | (s_pl[k].face < 0 ? 0 : s_pl[k].face == 4 ? 1 : 2));
  printf("], \"core\": [\"%a\", \"%a\", \"%a\", \"%a\"], \"tol_hex\": \"%a\", ", s_core[0] + s_mx, s_core[1] - s_mx, s_core[2] + s_mx,
         s_core[3] - s_mx, s_tol);
  printf("\"ground_stack\": 1, \"plane_stack\": 1, \"planes\": %d, \"draws\": %ld, \"served\": %ld, \"found\": %ld, \"edge_answers\": %ld, "
         "\"wrong\": %ld, \"not_general\": %ld, \"general_answers\": %ld, \"declined_of_general\": %ld, "
         "\"mx0_extra_answers\": %ld, \"mx0_wrong\": %ld, \"standing_off_changed\": %ld, \"standing_off_wrong\": %ld, "
         "\"coverage_rays\": %ld, \"coverage_general\": %ld, \"coverage_declined\": %ld, \"coverage_wrong\": %ld, \"mx\": %.17g, \"tol\": %.17g}\n",
         s_npl, n, served, found, edge_answers, ans_wrong, ans_not_general, general, declined, mx0_answers, mx0_wrong, stand_changed,
         stand_wrong, cov_rays, cov_general, cov_declined, cov_wrong, s_mx, s_tol);
  if (ans_wrong || ans_not_general || cov_wrong) return 1;
  if (coverage && !(cov_general > 0 && cov_declined * 100 <= cov_general)) return 4;
  return 0;
}
