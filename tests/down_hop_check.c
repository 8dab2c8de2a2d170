/* Adversarial CPU check of the down pass's decision (rt_device.h ground_hop_t<true>, trace.hip step 1'; DESIGN.md
 * §3.1): ground_hop's serve decision extended by the *found* hit — the closest hit among the ground primitives G is
 * no dielectric's, lies on an xz-rect (counted by the top of its padded box) or a RectBox y face at least `gap` below the top plane Y, at a
 * t above t_min, without a tie mark, under the same origin, |d.y| and slope conditions.  A found hit, like a served
 * one, must be the whole scene's closest hit by the reference's rules, in primitive, face and t.
 *
 * Everything the decision is judged by comes from tests/ground_hop_check.c, included here unchanged (its main
 * renamed): the reference's functions (oracle.c), the exhaustive closest hit with G tested first and last, the
 * reference's own walk of its own tree, the restated ground_stack record and the guard bitmap.  The decision itself
 * is restated below from those functions, not taken from the kernel.
 *
 *   down_hop_check <prims file> <draws> [seed [ties]]
 * Rays: ground_hop_check's draws (origins on, between and ulps either side of every plane of G, both directions,
 * slopes from straight down to 1e9, |d.y| around dy_min, hits at exactly t_min) and, one draw in four, a ray that
 * starts on or ulps off a plane of G and runs to another plane of G — the down pass's own segments.  Prints one JSON
 * line: how many rays were served and found, how many of each differ from the exhaustive answers and from the
 * reference's walk, and as controls how many found hits would differ with the "plane below Y" condition and with the
 * slope bounds switched off.  Exits 1 when a served or found ray differs (with `ties`: from the reference's walk
 * alone).  Test infrastructure (tests/test_down_hop.py); -ffp-contract=off. */
#define main ground_hop_check_main
#include "ground_hop_check.c"
#undef main

static double y_down;  /* Y - gap */

/* scene_compile.cpp ground_stack's gap = 4 eta + 4 tol, restated with ground_hop_check.c ground_stack's names */
static double stack_gap(void) {
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
  return 4.0 * eta + 4.0 * tol;
}

/* The extended decision: 0 refused, 1 served (a dielectric's RectBox y face: ground_hop_check.c serve), 2 found.
 * only_below / only_slope: a hit that the "plane below Y" condition / the slope bounds alone kept from being found. */
static int decide(const ray_t* r, double* t_best, int* best, int* face, int* only_below, int* only_slope) {
  int og, os, ot;
  *only_below = *only_slope = 0;
  const int sv = serve(r, t_best, best, face, &og, &os, &ot);  /* (also leaves G's closest hit in the outputs) */
  if (sv) return 1;
  if (*best < 0 || g_prims[*best].diel) return 0;
  /* serve() returns early on a tie mark without saying so: the closest hit in G again, with the mark */
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
  if (b != *best || f != *face || memcmp(&tb, t_best, sizeof tb)) { fprintf(stderr, "closest hit in G restated twice, two answers: %d %d %a, %d %d %a\n", b, f, tb, *best, *face, *t_best); exit(2); }
  if (tie || (f >= 0 && f < 4) || !(tb > T_MIN)) return 0;
  const double ay = fabs(r->d.y);
  if (!(r->o.y >= y_lo && r->o.y <= y_hi && ay > 0.0 && ay <= 0x1p300)) return 0;
  const int slope = ay >= dy_min && r->d.x * r->d.x + r->d.z * r->d.z <= ratio2 * (r->d.y * r->d.y);
  /* (a rect by the top of its padded leaf box, rect.rs:82-99: a raised rect whose box makes the top plane is on Y) */
  const double y = g_prims[b].kind == 3 ? g_prims[b].p[4] + 0.0001 : (f == 4 ? g_prims[b].p[4] : g_prims[b].p[1]);
  const int below = y <= y_down;
  *only_below = slope && !below;
  *only_slope = !slope && below;
  return (slope && below) ? 2 : 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  const long n = atol(argv[2]);
  if (argc > 3) s_state = (s_state + strtoull(argv[3], NULL, 0) * 0xD1B54A32D192ED03ull) | 1ull;
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
  const int ties = argc > 4 && !strcmp(argv[4], "ties");
  build_reference();
  if (!ground_stack()) { printf("{\"ground_stack\": 0}\n"); return 3; }
  y_down = y_top - stack_gap();
  int hop_down = 0;  /* ScenePlacement.hop_down restated: a non-dielectric member of G on a plane at or below y_down */
  for (int k = 0; k < g_ng; ++k) {
    const prim_c* q = &g_prims[g_g[k]];
    if (!q->diel) hop_down |= q->kind == 3 ? q->p[4] + 0.0001 <= y_down : (q->p[1] <= y_down || q->p[4] <= y_down);
  }
  int* sph = malloc(g_n * sizeof *sph), n_sph = 0;
  double pl[8], xlo = INFINITY, xhi = -INFINITY, zlo = INFINITY, zhi = -INFINITY;
  int n_pl = 0;
  for (int i = 0; i < g_n; ++i) {
    const double* p = g_prims[i].p;
    if (g_prims[i].kind == 0) { if (!never_hit(p)) sph[n_sph++] = i; continue; }
    if (g_prims[i].kind == 4) { pl[n_pl++] = p[1]; pl[n_pl++] = p[4]; xlo = fmin(xlo, p[0]); xhi = fmax(xhi, p[3]); zlo = fmin(zlo, p[2]); zhi = fmax(zhi, p[5]); }
    else { pl[n_pl++] = p[4]; xlo = fmin(xlo, p[0]); xhi = fmax(xhi, p[1]); zlo = fmin(zlo, p[2]); zhi = fmax(zhi, p[3]); }
  }
  long served = 0, found = 0, served_wrong = 0, found_wrong = 0, served_wrong_ref = 0, found_wrong_ref = 0;
  long not_below = 0, wrong_not_below = 0, not_slope = 0, wrong_not_slope = 0, found_at_t_min_refused = 0, found_up = 0;
  for (long it = 0; it < n; ++it) {
    int mode = (int)(next_u64() % 8);
    if (!n_sph && mode != 0 && mode != 2 && mode != 7) {  /* a stack without spheres: no contact-point draws */
      static const int other[3] = {0, 2, 7};
      mode = other[next_u64() % 3];
    }
    const double* sp = n_sph ? g_prims[sph[next_u64() % (uint64_t)n_sph]].p : NULL;
    ray_t r;
    /* origin height: on a plane, ulps around it, or between two planes */
    const double plane = pl[next_u64() % (uint64_t)n_pl];
    const int hm = (int)(next_u64() % 6);
    r.o.y = hm == 0 ? plane : hm == 1 ? ulps(plane, (int)(next_u64() % 9) - 4) : hm == 2 ? plane + range(-1e-12, 1e-12)
            : hm == 3 ? range(y_lo, y_hi) : hm == 4 ? plane + (unif() < 0.5 ? -1.0 : 1.0) * logu(1e-15, 1e-3) : plane;
    /* origin xz */
    if (mode == 0 || (mode == 7 && !sp)) { r.o.x = range(xlo, xhi); r.o.z = range(zlo, zhi); }
    else if (mode == 1) { r.o.x = sp[0]; r.o.z = sp[2]; if (unif() < 0.5) { r.o.x = ulps(r.o.x, (int)(next_u64() % 5) - 2); r.o.z += range(-1e-9, 1e-9); } }
    else if (mode == 2) { const double e = logu(1e-12, 1e-2); r.o.x = (unif() < 0.5 ? xlo : xhi) + range(-e, e); r.o.z = (unif() < 0.5 ? zlo : zhi) + range(-e, e); if (unif() < 0.5) r.o.z = range(zlo, zhi); }
    else { const double rho = mode == 3 ? logu(1e-6, 0.5) : logu(1e-3, 8.0), a = range(0.0, 6.283185307179586); r.o.x = sp[0] + rho * cos(a); r.o.z = sp[2] + rho * sin(a); }
    /* direction */
    if (mode >= 3 && mode <= 6) {  /* aimed at a contact point, offset by 1e-17 .. 1e-1, at or just around the top plane */
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
      /* the pass's own segments: from on or ulps off one plane of G towards another, the slope around R (2^10) or
       * |d.y| around dy_min one time in two */
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
    if (mode == 7) {  /* a ground hit just around t_min: the origin 0.001 |d.y| (1 +- small) from a plane */
      const double target = pl[next_u64() % (uint64_t)n_pl];
      r.o.y = target - r.d.y * T_MIN * (1.0 + range(-1e-9, 1e-9) * (double)(next_u64() % 3));
    }
    double t, te; int b, fc, be, fe, ob, os;
    const int kind = decide(&r, &t, &b, &fc, &ob, &os);
    if (!kind && !ob && !os) {
      if (b >= 0 && !g_prims[b].diel && !(t > T_MIN) && t == T_MIN) ++found_at_t_min_refused;
      continue;
    }
    int diff = 0;
    for (int gf = 0; gf < 2; ++gf) {
      exhaustive(&r, gf, &te, &be, &fe);
      diff |= !(be == b && fe == fc && te == t);
    }
    reference(&r, &te, &be, &fe);
    const int dr = !(be == b && fe == fc && te == t);
    if (kind == 1) { ++served; served_wrong += diff; served_wrong_ref += dr; }
    if (kind == 2) { ++found; found_wrong += diff; found_wrong_ref += dr; found_up += r.d.y > 0.0; }
    if (ob) { ++not_below; wrong_not_below += ties ? dr : diff; }
    if (os) { ++not_slope; wrong_not_slope += ties ? dr : diff; }
    if (kind && (ties ? dr : (diff || dr)) && served_wrong + found_wrong + served_wrong_ref + found_wrong_ref <= 8)
      fprintf(stderr, "%s ray differs: o %a %a %a d %a %a %a: ground %d face %d t %a, reference %d face %d t %a\n",
              kind == 1 ? "served" : "found", r.o.x, r.o.y, r.o.z, r.d.x, r.d.y, r.d.z, b, fc, t, be, fe, te);
  }
  printf("{\"ground_stack\": 1, \"hop_down\": %d, \"draws\": %ld, \"served\": %ld, \"found\": %ld, \"found_upward\": %ld, "
         "\"served_wrong\": %ld, \"found_wrong\": %ld, \"served_wrong_reference\": %ld, \"found_wrong_reference\": %ld, "
         "\"refused_not_below\": %ld, \"wrong_without_below\": %ld, \"refused_by_slope\": %ld, \"wrong_without_slope\": %ld, "
         "\"refused_at_t_min\": %ld, \"y_down\": %.17g}\n",
         hop_down, n, served, found, found_up, served_wrong, found_wrong, served_wrong_ref, found_wrong_ref, not_below,
         wrong_not_below, not_slope, wrong_not_slope, found_at_t_min_refused, y_down);
  return (served_wrong_ref || found_wrong_ref || ((served_wrong || found_wrong) && !ties)) ? 1 : 0;
}
