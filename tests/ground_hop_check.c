/* Adversarial CPU check of the ground-stack hop pass (rt_device.h ground_hop, scene_compile.cpp ground_stack;
 * DESIGN.md §3.1): whenever the pass would serve a ray — the closest hit among the ground primitives G alone,
 * under the record's conditions — that hit must be the whole scene's closest hit by the reference's rules, in
 * primitive, face and t.  The serve decision is restated here from the reference's own functions (oracle.c,
 * included unchanged: aabb_hit2, rect_hit, sphere_hit), with the constants of ground_stack; the exhaustive answer
 * tests every primitive as bbox_tree.rs:60-71 does a leaf (hit2 on its bounding box, then the object, against the
 * running closest), once with G tested first and once with G tested last, so a sphere meets both the largest
 * and the smallest t_max any tree order can give it; a served ray must agree with both (`served_wrong`).  It must
 * also agree with the reference's own answer — the rhs-first walk (oracle.c tree_hit) of the tree oracle.c builds
 * from the primitives in file order, which is the scene's object order (`served_wrong_reference`).  That walk also
 * judges a stack with exact ties inside G (a rect on a RectBox's face, a RectBox twice), which the two orders
 * cannot: which tied primitive wins depends on the tree's leaf order, the order the device numbers
 * its primitives in and the serve decision below compares by.  With `ties` the exit status follows the walk alone.
 *
 *   ground_hop_check <prims file> <draws> [seed [ties]]
 * prims file: one line per primitive, `kind dielectric p0 .. p5` (kind 0 sphere, 3 XZ rect, 4 RectBox; C99 hex
 * floats).  Rays: origins on, between and an ulp or a few either side of G's planes, at and around contact
 * points, near G's edges; directions from straight down to |d.y| = 1e-9 |d|, scaled off unit length, many aimed
 * at a contact point offset by 1e-17 .. 1e-1; hits closer than t_min (a stack without spheres has no contact
 * point: its draws are the others).  Prints the counts as one JSON line — also how many served answers would
 * differ with the guard bitmap, with the slope bounds, and with the refusal of a hit at exactly t_min, switched
 * off — and exits 1 when a served ray differs.  Test infrastructure (tests/test_ground_hop.py); -ffp-contract=off. */
#include "../oracle/oracle.c"

#include <stdio.h>

#define CELLS 32.0
#define CELL (1.0 / 32.0)
#define GUARD (1.0 / 32.0)

typedef struct prim_c {
  int kind, diel;
  double p[6];
} prim_c;
static prim_c* g_prims;
static int g_n, g_ng, g_nbox, g_g[4];
static double y_lo, y_hi, y_top, dy_min, ratio2, gx0, gz0;
static int gnx, gnz;
static unsigned* g_bits;
static const double T_MIN = 0.001;

static uint64_t s_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64(void) {
  uint64_t x = s_state;
  x ^= x << 13; x ^= x >> 7; x ^= x << 17;
  return s_state = x;
}
static double unif(void) { return (double)(next_u64() >> 11) * 0x1p-53; }
static double range(double a, double b) { return a + (b - a) * unif(); }
static double logu(double a, double b) { return exp(range(log(a), log(b))); }
static double ulps(double x, int k) {
  for (; k > 0; --k) x = nextafter(x, INFINITY);
  for (; k < 0; ++k) x = nextafter(x, -INFINITY);
  return x;
}

/* The reference's own tree over the primitives (oracle.c or_scene_new: constructor.rs:9-36) and every primitive's
 * place in its leaf order, lhs before rhs — the number the device gives it (scene_compile.cpp reference_ranks),
 * which ground_stack lists G by and tie_takes compares. */
static or_scene* g_ref;
static work_t g_work;
static int *g_rank, *g_by_rank;
static void build_reference(void) {
  rt_object* objs = calloc((size_t)g_n, sizeof *objs);
  for (int i = 0; i < g_n; ++i) {
    objs[i].geometry = g_prims[i].kind == 0 ? RT_GEOM_SPHERE : g_prims[i].kind == 3 ? RT_GEOM_RECT_XZ : RT_GEOM_RECT_BOX;
    for (int k = 0; k < 6; ++k) objs[i].p[k] = g_prims[i].p[k];
  }
  rt_scene_desc d;
  memset(&d, 0, sizeof d);
  d.n_objects = g_n;
  d.objects = objs;
  g_ref = or_scene_new(&d);
  free(objs);
  work_init(g_ref, &g_work);
  g_rank = malloc((size_t)g_n * sizeof *g_rank);
  g_by_rank = malloc((size_t)g_n * sizeof *g_by_rank);
  int32_t* stack = malloc((size_t)(g_ref->n_tree + 2) * sizeof *stack);
  int sp = 0, next = 0;
  if (g_ref->root >= 0) stack[sp++] = g_ref->root;
  while (sp > 0) {
    const node_t* nd = &g_ref->tree[stack[--sp]];
    if (nd->leaf >= 0) { g_rank[nd->leaf] = next; g_by_rank[next++] = nd->leaf; continue; }
    stack[sp++] = nd->rhs;  /* (popped after the whole lhs subtree) */
    stack[sp++] = nd->lhs;
  }
  free(stack);
}

static int never_hit(const double* p) { return p[3] <= 0.0 && p[1] - p[3] >= p[1] + p[3]; }
static int cell_of(double v, double v0, int n) {  /* rt_layout.h ground_cell */
  const double q = (v - v0) * CELLS;
  return (q >= 0.0 && q < (double)n) ? (int)q : -1;
}

/* scene_compile.cpp ground_stack, restated; 0 when the scene has no ground stack */
static int ground_stack(void) {
  double top = -INFINITY, low = INFINITY, ex0 = INFINITY, ex1 = -INFINITY, ez0 = INFINITY, ez1 = -INFINITY;
  double r_min = INFINITY, r_max = 0.0, planes[8];
  int n_planes = 0, boxes[4], rects[4], nb = 0, nr = 0;
  for (int k = 0; k < g_n; ++k) {  /* (in the device's numbering: G is listed boxes first, each kind by rank) */
    const int i = g_by_rank[k];
    const double* p = g_prims[i].p;
    if (g_prims[i].kind == 4) {
      if (nb + nr == 4) return 0;
      boxes[nb++] = i;
      planes[n_planes++] = p[1]; planes[n_planes++] = p[4];
      top = fmax(top, p[4]);
      ex0 = fmin(ex0, p[0]); ex1 = fmax(ex1, p[3]); ez0 = fmin(ez0, p[2]); ez1 = fmax(ez1, p[5]);
    } else if (g_prims[i].kind == 3) {
      if (nb + nr == 4) return 0;
      rects[nr++] = i;
      planes[n_planes++] = p[4];
      top = fmax(top, p[4] + 0.0001);
      ex0 = fmin(ex0, p[0]); ex1 = fmax(ex1, p[1]); ez0 = fmin(ez0, p[2]); ez1 = fmax(ez1, p[3]);
    } else if (g_prims[i].kind == 0) {
      if (never_hit(p)) continue;
      if (!(p[3] > 0.0)) return 0;
      r_min = fmin(r_min, p[3]); r_max = fmax(r_max, p[3]);
    } else {
      return 0;
    }
  }
  if (nb + nr < 1) return 0;
  for (int i = 0; i < n_planes; ++i) low = fmin(low, planes[i]);
  double dist = 0.0;
  for (int i = 0; i < g_n; ++i) {
    const double* p = g_prims[i].p;
    if (g_prims[i].kind != 0 || never_hit(p)) continue;
    if (!(p[1] - p[3] >= top)) return 0;
    const double dx = fmax(fabs(p[0] - ex0), fabs(p[0] - ex1)), dy = fmax(fabs(p[1] - low), fabs(p[1] - top));
    const double dz = fmax(fabs(p[2] - ez0), fabs(p[2] - ez1));
    dist = fmax(dist, sqrt(dx * dx + dy * dy + dz * dz));
  }
  const double ratio = 0x1p10, tol = 0x1p-40 * fmax(1.0, fmax(fabs(top), fabs(low)));
  const double reach = ((top - low) + 2.0 * tol) * (ratio + 1.0);
  const double l2 = (dist + reach) * (dist + reach) + reach * reach + r_max * r_max;
  const double eta = isfinite(r_min) ? 0x1p-38 * l2 / (2.0 * r_min) : 0.0;
  if (!(eta <= 0x1p-16 && 0x1p-38 * l2 <= 0x1p-13)) return 0;
  for (int i = 0; i < n_planes; ++i)
    if (planes[i] != top && !(planes[i] <= top - (4.0 * eta + 4.0 * tol))) return 0;
  y_lo = low - tol; y_hi = top + tol; y_top = top;
  dy_min = fmax((2.0 * eta + 4.0 * tol) / 0.001, 0x1p-100);
  ratio2 = ratio * ratio;
  g_ng = nb + nr; g_nbox = nb;
  for (int i = 0; i < nb; ++i) g_g[i] = boxes[i];
  for (int i = 0; i < nr; ++i) g_g[nb + i] = rects[i];
  /* the guard bitmap */
  double cx0 = INFINITY, cx1 = -INFINITY, cz0 = INFINITY, cz1 = -INFINITY;
  for (int i = 0; i < g_n; ++i) {
    const double* p = g_prims[i].p;
    if (g_prims[i].kind != 0 || never_hit(p) || !((p[1] - p[3]) - top < GUARD / 2)) continue;
    cx0 = fmin(cx0, p[0]); cx1 = fmax(cx1, p[0]); cz0 = fmin(cz0, p[2]); cz1 = fmax(cz1, p[2]);
  }
  gnx = gnz = 0;
  if (!isfinite(cx0)) return 1;
  gx0 = floor(cx0 * CELLS - 2.0) * CELL; gz0 = floor(cz0 * CELLS - 2.0) * CELL;
  gnx = (int)ceil((cx1 - gx0) * CELLS + 2.0); gnz = (int)ceil((cz1 - gz0) * CELLS + 2.0);
  g_bits = calloc(((size_t)gnx * gnz + 31) / 32, 4);
  const double rad = GUARD * (1.0 + 0x1p-20);
  for (int s = 0; s < g_n; ++s) {
    const double* p = g_prims[s].p;
    if (g_prims[s].kind != 0 || never_hit(p) || !((p[1] - p[3]) - top < GUARD / 2)) continue;
    const int i0 = cell_of(p[0], gx0, gnx), k0 = cell_of(p[2], gz0, gnz);
    for (int k = k0 - 3; k <= k0 + 3; ++k)
      for (int i = i0 - 3; i <= i0 + 3; ++i) {
        if (i < 0 || k < 0 || i >= gnx || k >= gnz) continue;
        const double xl = gx0 + i * CELL, zl = gz0 + k * CELL;
        const double dx = fmax(0.0, fmax(xl - p[0], p[0] - (xl + CELL))), dz = fmax(0.0, fmax(zl - p[2], p[2] - (zl + CELL)));
        if (dx * dx + dz * dz <= rad * rad) {
          const size_t c = (size_t)k * gnx + i;
          g_bits[c >> 5] |= 1u << (c & 31);
        }
      }
  }
  return 1;
}

static aabb_t leaf_box_of(const prim_c* q) {  /* sphere.rs:54-60, rect.rs:82-99, rect.rs:158-163 */
  const double* p = q->p;
  double b[6];
  if (q->kind == 0) { b[0] = p[0] - p[3]; b[1] = p[1] - p[3]; b[2] = p[2] - p[3]; b[3] = p[0] + p[3]; b[4] = p[1] + p[3]; b[5] = p[2] + p[3]; }
  else if (q->kind == 3) { b[0] = p[0]; b[1] = p[4] - 0.0001; b[2] = p[2]; b[3] = p[1]; b[4] = p[4] + 0.0001; b[5] = p[3]; }
  else { for (int k = 0; k < 6; ++k) b[k] = p[k]; }
  return box_from(b);
}
/* rect.rs:146-156 RectBox::hit with the face index (oracle.c rectbox_hit's loop) */
static int box_hit_face(const double* b, const ray_t* r, double t_min, double t_max, double* t_out) {
  const double sides[6][5] = {{b[0], b[3], b[1], b[4], b[5]}, {b[0], b[3], b[1], b[4], b[2]}, {b[1], b[4], b[2], b[5], b[3]},
                              {b[1], b[4], b[2], b[5], b[0]}, {b[0], b[3], b[2], b[5], b[4]}, {b[0], b[3], b[2], b[5], b[1]}};
  static const int d1[6] = {0, 0, 1, 1, 0, 0}, d2[6] = {1, 1, 2, 2, 2, 2};
  int face = -1;
  double tc = t_max;
  for (int s = 0; s < 6; ++s) {
    hit_t h;
    if (rect_hit(d1[s], d2[s], sides[s], r, t_min, tc, &h)) { tc = h.t; face = s; }
  }
  *t_out = tc;
  return face;
}
/* one leaf by the reference's rule against the running closest; 1 when it becomes the closest */
static int leaf_test(int i, const ray_t* r, double* t_best, int* best, int* face) {
  const prim_c* q = &g_prims[i];
  if (!aabb_hit2(leaf_box_of(q), r, T_MIN, *t_best)) return 0;
  double t;
  int f = -1;
  hit_t h;
  if (q->kind == 0) { if (!sphere_hit(q->p, r, T_MIN, *t_best, &h)) return 0; t = h.t; }
  else if (q->kind == 3) { if (!rect_hit(0, 2, q->p, r, T_MIN, *t_best, &h)) return 0; t = h.t; }
  else { f = box_hit_face(q->p, r, T_MIN, *t_best, &t); if (f < 0) return 0; }
  *t_best = t; *best = i; *face = f;
  return 1;
}
static int in_g(int i) { return g_prims[i].kind != 0; }
static void exhaustive(const ray_t* r, int g_first, double* t, int* best, int* face) {
  *t = INFINITY; *best = -1; *face = -1;
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i < g_n; ++i)
      if (in_g(i) == ((pass == 0) == (g_first != 0))) leaf_test(i, r, t, best, face);
}
/* the reference's own answer: its rhs-first walk of its own tree (oracle.c tree_hit: bbox_tree.rs:56-91), which
 * also decides which of several primitives hit at exactly the closest t wins */
static void reference(const ray_t* r, double* t, int* best, int* face) {
  hit_t h;
  int32_t obj = -1;
  *t = INFINITY; *best = -1; *face = -1;
  if (!tree_hit(g_ref, &g_work, r, T_MIN, INFINITY, &h, &obj)) return;
  *t = h.t; *best = obj;
  /* (RectBox::hit keeps the last of its sides at the closest t, whatever t_max >= t it was called with) */
  if (g_prims[obj].kind == 4) { double tf; *face = box_hit_face(g_prims[obj].p, r, T_MIN, h.t, &tf); }
}

/* rt_device.h ground_hop restated: 0 not served; 1 served; the flags say which condition alone refused it */
static int near_entry(double te, double tb) {
  uint64_t a, b;
  memcpy(&a, &te, 8); memcpy(&b, &tb, 8);
  return (unsigned)(a >> 32) - (unsigned)(b >> 32) <= 1u;
}
static double slab_entry(aabb_t b, const ray_t* r, double t_min) {  /* hit2's entry, without the early return */
  for (int a = 0; a < 3; ++a) {
    const double inv = 1.0 / vget(r->d, a);
    double t0 = (vget(b.mn, a) - vget(r->o, a)) * inv, t1 = (vget(b.mx, a) - vget(r->o, a)) * inv;
    if (inv < 0.0) t0 = t1;
    t_min = (t0 > t_min) ? t0 : t_min;
  }
  return t_min;
}
static int serve(const ray_t* r, double* t_best, int* best, int* face, int* only_guard, int* only_slope, int* only_t_min) {
  int tie = 0;
  *t_best = INFINITY; *best = -1; *face = -1; *only_guard = *only_slope = *only_t_min = 0;
  for (int k = 0; k < g_ng; ++k) {
    const int i = g_g[k];
    const prim_c* q = &g_prims[i];
    const aabb_t lb = leaf_box_of(q);
    if (!aabb_hit2(lb, r, T_MIN, *t_best)) {
      if (k < g_nbox && *best >= 0 && near_entry(slab_entry(lb, r, T_MIN), *t_best)) tie = 1;  /* mark_tie */
      continue;
    }
    double t;
    int f = -1;
    hit_t h;
    if (k < g_nbox) { f = box_hit_face(q->p, r, T_MIN, *t_best, &t); if (f < 0) continue; }
    else { if (!rect_hit(0, 2, q->p, r, T_MIN, *t_best, &h)) continue; t = h.t; }
    if (t == *t_best && *best >= 0) {  /* tie_takes */
      if (tie) continue;
      if (!(g_rank[i] < g_rank[*best]) && aabb_hit2(leaf_box_of(&g_prims[*best]), r, T_MIN, t)) continue;
    }
    *t_best = t; *best = i; *face = f; tie = 0;
  }
  if (*best < 0 || tie || *face < 4 || !g_prims[*best].diel) return 0;
  const int at_t_min = !(*t_best > T_MIN);  /* (a hit at exactly t_min is not served) */
  const double ay = fabs(r->d.y);
  if (!(r->o.y >= y_lo && r->o.y <= y_hi && ay > 0.0 && ay <= 0x1p300)) return 0;
  const int slope = ay >= dy_min && r->d.x * r->d.x + r->d.z * r->d.z <= ratio2 * (r->d.y * r->d.y);
  int guarded = 0;
  if ((*face == 4 ? g_prims[*best].p[4] : g_prims[*best].p[1]) == y_top) {
    const int ix = cell_of(r->o.x + *t_best * r->d.x, gx0, gnx), iz = cell_of(r->o.z + *t_best * r->d.z, gz0, gnz);
    if (ix >= 0 && iz >= 0) {
      const size_t c = (size_t)iz * gnx + ix;
      guarded = (g_bits[c >> 5] >> (c & 31)) & 1u;
    }
  }
  *only_guard = slope && guarded && !at_t_min;
  *only_slope = !slope && !guarded && !at_t_min;
  *only_t_min = slope && !guarded && at_t_min;
  return slope && !guarded && !at_t_min;
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
  int* sph = malloc(g_n * sizeof *sph), n_sph = 0;
  double pl[8], xlo = INFINITY, xhi = -INFINITY, zlo = INFINITY, zhi = -INFINITY;
  int n_pl = 0;
  for (int i = 0; i < g_n; ++i) {
    const double* p = g_prims[i].p;
    if (g_prims[i].kind == 0) { if (!never_hit(p)) sph[n_sph++] = i; continue; }
    if (g_prims[i].kind == 4) { pl[n_pl++] = p[1]; pl[n_pl++] = p[4]; xlo = fmin(xlo, p[0]); xhi = fmax(xhi, p[3]); zlo = fmin(zlo, p[2]); zhi = fmax(zhi, p[5]); }
    else { pl[n_pl++] = p[4]; xlo = fmin(xlo, p[0]); xhi = fmax(xhi, p[1]); zlo = fmin(zlo, p[2]); zhi = fmax(zhi, p[3]); }
  }
  long served = 0, wrong = 0, wrong_no_guard = 0, wrong_no_slope = 0, refused_guard = 0, refused_slope = 0, top_exits = 0;
  long sphere_wins = 0, wrong_ref = 0, refused_t_min = 0, wrong_no_t_min = 0;
  double worst_rho = 0.0;
  for (long it = 0; it < n; ++it) {
    int mode = (int)(next_u64() % 8);
    if (!n_sph && mode != 0 && mode != 2 && mode != 7) {  /* a stack without spheres: no contact-point draws */
      static const int other[3] = {0, 2, 7};
      mode = other[next_u64() % 3];
    }
    const double* sp = n_sph ? g_prims[sph[next_u64() % (uint64_t)n_sph]].p : NULL;  /* a sphere: its contact point (sp[0], y_top, sp[2]) */
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
    double tx, ty, tz;
    if (mode >= 3 && mode <= 6) {  /* aimed at a contact point, offset by 1e-17 .. 1e-1, at or just around the top plane */
      const double off = logu(1e-17, 1e-1), a = range(0.0, 6.283185307179586);
      const int vm = (int)(next_u64() % 4);
      tx = sp[0] + off * cos(a); tz = sp[2] + off * sin(a);
      ty = vm == 0 ? y_top : vm == 1 ? ulps(y_top, (int)(next_u64() % 5) - 2) : vm == 2 ? y_top + logu(1e-17, 1e-6) : y_top - logu(1e-17, 1e-6);
      r.d = V(tx - r.o.x, ty - r.o.y, tz - r.o.z);
      if (mode == 6) r.d.y = (unif() < 0.5 ? -1.0 : 1.0) * logu(1e-9, 1e-2) * sqrt(r.d.x * r.d.x + r.d.z * r.d.z);  /* grazing past it */
    } else {
      const double a = range(0.0, 6.283185307179586), sy = (unif() < 0.5 ? -1.0 : 1.0) * (unif() < 0.5 ? logu(1e-9, 1.0) : range(0.0, 1.0));
      const double sxz = sqrt(fmax(0.0, 1.0 - sy * sy));
      r.d = V(sxz * cos(a), sy, sxz * sin(a));
    }
    const double sc = (next_u64() & 3) == 0 ? logu(1e-3, 1e3) : range(0.5, 2.0);
    r.d = vscale(r.d, sc);
    if (mode == 7) {  /* a ground hit just around t_min: the origin 0.001 |d.y| (1 +- small) from a plane */
      const double target = pl[next_u64() % (uint64_t)n_pl];
      r.o.y = target - r.d.y * T_MIN * (1.0 + range(-1e-9, 1e-9) * (double)(next_u64() % 3));
    }
    double t, te; int b, fc, be, fe, og, os, ot;
    const int sv = serve(&r, &t, &b, &fc, &og, &os, &ot);
    if (!sv && !og && !os && !ot) continue;
    int diff = 0;
    for (int gf = 0; gf < 2; ++gf) {
      exhaustive(&r, gf, &te, &be, &fe);
      diff |= !(be == b && fe == fc && te == t);
    }
    if (fc == 4 && g_prims[b].p[4] == y_top) top_exits += sv || og;
    if (sv || ot) {
      if (sv) { ++served; wrong += diff; }
      reference(&r, &te, &be, &fe);
      const int dr = !(be == b && fe == fc && te == t);
      if (sv) wrong_ref += dr;
      else { ++refused_t_min; wrong_no_t_min += dr; }
      if (sv && dr && wrong_ref <= 5)
        fprintf(stderr, "served ray differs from the reference: o %a %a %a d %a %a %a: ground %d face %d t %a, reference %d face %d t %a\n",
                r.o.x, r.o.y, r.o.z, r.d.x, r.d.y, r.d.z, b, fc, t, be, fe, te);
    }
    if (og) { ++refused_guard; wrong_no_guard += diff; }
    if (os) { ++refused_slope; wrong_no_slope += diff; }
    if (diff && be >= 0 && g_prims[be].kind == 0) {
      ++sphere_wins;
      if (og) {
        const double ex = r.o.x + t * r.d.x - g_prims[be].p[0], ez = r.o.z + t * r.d.z - g_prims[be].p[2];
        worst_rho = fmax(worst_rho, sqrt(ex * ex + ez * ez));
      }
    }
    if (sv && diff && wrong <= 5 && !ties)
      fprintf(stderr, "served ray differs: o %a %a %a d %a %a %a: ground %d face %d t %a, exhaustive %d face %d t %a\n", r.o.x,
              r.o.y, r.o.z, r.d.x, r.d.y, r.d.z, b, fc, t, be, fe, te);
  }
  printf("{\"ground_stack\": 1, \"draws\": %ld, \"served\": %ld, \"served_wrong\": %ld, \"refused_by_guard\": %ld, "
         "\"wrong_without_guard\": %ld, \"refused_by_slope\": %ld, \"wrong_without_slope\": %ld, \"top_exits\": %ld, "
         "\"sphere_wins\": %ld, \"largest_flip_distance\": %.3g, \"dy_min\": %.3g, \"served_wrong_reference\": %ld, "
         "\"refused_at_t_min\": %ld, \"wrong_reference_without_t_min\": %ld}\n",
         n, served, wrong, refused_guard, wrong_no_guard, refused_slope, wrong_no_slope, top_exits, sphere_wins, worst_rho, dy_min,
         wrong_ref, refused_t_min, wrong_no_t_min);
  return (wrong_ref || (wrong && !ties)) ? 1 : 0;
}
