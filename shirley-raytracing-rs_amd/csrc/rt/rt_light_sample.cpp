// rt_light_sample.cpp — solid-angle sampling of sphere and rect lights in include/shirley_rt.h (added within ABI 11;
// light_cone.h, light_rect.h, direct.h, nee.hip, direct.hip's light_sample_kernel): the scene
// setting, the device probe of one light sample per vertex, and the same sample in plain C++ without a device.
#include "rt_ctx.h"
#include "light_cone.h"
#include "light_rect.h"

using namespace rt;

namespace {

constexpr double kPi = 3.141592653589793;
// (the launchers take the mode's value as their instances' sample kind)
static_assert(kSampleArea == RT_LIGHT_SAMPLE_AREA && kSampleCone == RT_LIGHT_SAMPLE_SOLID_ANGLE &&
                  kSampleAll == RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL,
              "sample kinds are the public modes");

// The grid pick of light_pick.h on the host table: the vertex's cell, the smallest k with xi < cdf_k, its p.
int host_cell_axis(double x, double lo, double hi, int n) {
  const double inv = n == 1 ? 0.0 : (double)n / (hi - lo);
  const double q = (x - lo) * inv;
  return !(q >= 0.0) ? 0 : q >= (double)n ? n - 1 : (int)q;
}

int host_grid_pick(const LightGridTable& t, const double* x, double xi, double* prob) {
  const rt_light_grid& g = t.info;
  const int ix = host_cell_axis(x[0], g.lo[0], g.hi[0], g.n[0]);
  const int iy = host_cell_axis(x[1], g.lo[1], g.hi[1], g.n[1]);
  const int iz = host_cell_axis(x[2], g.lo[2], g.hi[2], g.n[2]);
  const double* row = t.cdf.data() + (size_t)((iz * g.n[1] + iy) * g.n[0] + ix) * (size_t)g.n_lights;
  int k = 0;
  while (k < g.n_lights - 1 && !(xi < row[k])) ++k;
  *prob = row[k] - (k ? row[k - 1] : 0.0);
  return k;
}

double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// One vertex of rt_light_sample_host: the header's light sample up to the shadow ray, with a = 1.
void host_light_sample(const std::vector<DLight>& lights, const LightGridTable* grid, int mode, uint64_t seed,
                       uint32_t pixel, const double* x, const double* n, rt_light_sample* out) {
  const int L = (int)lights.size();
  const double nl = (double)L;
  uint32_t draw = 0;
  auto next = [&] { return path_draw(seed, pixel, 0u, draw++); };
  double pk = 1.0;
  int li;
  if (grid) {
    li = host_grid_pick(*grid, x, next(), &pk);
  } else {
    const int pick = (int)(next() * nl);
    li = pick < L - 1 ? pick : L - 1;
  }
  const DLight& Lt = lights[li];
  const int geom = Lt.geometry;
  const bool solid_angle = mode != RT_LIGHT_SAMPLE_AREA && geom == RT_GEOM_SPHERE;
  bool rect_angle = false;  // a rect's sample came from its spherical rectangle, of solid angle om
  rt_light_sample r{};
  r.light = li;
  double w[3], u[3] = {0.0, 0.0, 0.0}, om = 0.0;
  if (mode == RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL && geom != RT_GEOM_SPHERE) {
    const int d1 = geom == RT_GEOM_RECT_YZ ? 1 : 0, d2 = geom == RT_GEOM_RECT_XY ? 1 : 2, ax = 3 - d1 - d2;
    RectView rv;
    const int open = rect_open(Lt.p, x[d1], x[d2], x[ax], rv);
    if (open == kRectCoplanar) {
      r.flags = 4;
      r.draws = draw;
      *out = r;
      return;
    }
    const double xi1 = next();
    const double xi2 = next();
    if (open == kRectOpen) {
      rect_angle = true;
      om = rv.S;
      rect_sample(rv, xi1, xi2, w[d1], w[d2], w[ax]);
    } else {  // the area form's point on the same two draws
      r.flags = 8;
      w[d1] = (Lt.p[0] + xi1 * (Lt.p[1] - Lt.p[0])) - x[d1];
      w[d2] = (Lt.p[2] + xi2 * (Lt.p[3] - Lt.p[2])) - x[d2];
      w[ax] = Lt.p[4] - x[ax];
    }
  } else if (solid_angle) {
    const c3 c{Lt.p[0], Lt.p[1], Lt.p[2]}, xv{x[0], x[1], x[2]};
    c3 wc, cw, cu;
    double dc2;
    if (!cone_open(c, Lt.p[3], xv, wc, dc2, om)) {
      r.flags = 2;
      r.draws = draw;
      *out = r;
      return;
    }
    double px, py;
    do {  // random_in_unit_disk
      px = -1.0 + 2.0 * next();
      py = -1.0 + 2.0 * next();
    } while (!(px * px + py * py <= 1.0));
    cone_sample(c, Lt.p[3], xv, wc, dc2, om, px, py, cw, cu);
    w[0] = cw.x, w[1] = cw.y, w[2] = cw.z;
    u[0] = cu.x, u[1] = cu.y, u[2] = cu.z;
  } else {
    double y[3];
    if (geom == RT_GEOM_SPHERE) {
      double p[3];
      do {  // random_in_unit_sphere
        p[0] = -1.0 + 2.0 * next();
        p[1] = -1.0 + 2.0 * next();
        p[2] = -1.0 + 2.0 * next();
      } while (!(dot3(p, p) <= 1.0));
      const double ln = __builtin_sqrt(dot3(p, p));
      for (int a = 0; a < 3; ++a) {
        u[a] = p[a] / ln;
        y[a] = Lt.p[a] + u[a] * Lt.p[3];
      }
    } else {
      const double xi1 = next();
      const double xi2 = next();
      const double c1 = Lt.p[0] + xi1 * (Lt.p[1] - Lt.p[0]);
      const double c2 = Lt.p[2] + xi2 * (Lt.p[3] - Lt.p[2]);
      const int d1 = geom == RT_GEOM_RECT_YZ ? 1 : 0, d2 = geom == RT_GEOM_RECT_XY ? 1 : 2;
      y[d1] = c1;
      y[d2] = c2;
      y[3 - d1 - d2] = Lt.p[4];
    }
    for (int a = 0; a < 3; ++a) w[a] = y[a] - x[a];
  }
  const double d2 = dot3(w, w);
  const double dist = __builtin_sqrt(d2);
  const double cx = dot3(n, w) / dist;
  double cy;
  if (geom == RT_GEOM_SPHERE) {
    cy = -dot3(u, w) / dist;
  } else {
    const double wa = geom == RT_GEOM_RECT_XY ? w[2] : geom == RT_GEOM_RECT_YZ ? w[0] : w[1];
    cy = __builtin_fabs(wa) / dist;
  }
  r.draws = draw;
  for (int a = 0; a < 3; ++a) r.w[a] = w[a];
  r.cx = cx;
  r.cy = cy;
  if (!(cx > 0.0 && cy > 0.0)) {
    r.flags |= 1;
  } else if (rect_angle) {
    r.g_plain = cx * ((grid ? om / pk : om * nl) / kPi);
    const double gs = cx / kPi;
    const double pl = grid ? pk / om : 1.0 / (om * nl);
    r.g_mis = gs / (pl + gs);
  } else if (solid_angle) {
    r.g_plain = cx * (grid ? (2.0 * om) / pk : (2.0 * om) * nl);
    const double gs = cx / kPi;
    const double pl = grid ? pk / ((2.0 * kPi) * om) : 1.0 / (((2.0 * kPi) * om) * nl);
    r.g_mis = gs / (pl + gs);
  } else {
    r.g_plain = ((cx * cy) / d2) * ((grid ? Lt.area / pk : Lt.area * nl) / kPi);
    const double gs = ((cx * cy) / d2) / kPi;
    const double pl = grid ? pk / Lt.area : 1.0 / (Lt.area * nl);
    r.g_mis = gs / (pl + gs);
  }
  *out = r;
}

bool known_mode(int32_t mode) {
  return mode == RT_LIGHT_SAMPLE_AREA || mode == RT_LIGHT_SAMPLE_SOLID_ANGLE || mode == RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL;
}

}  // namespace

extern "C" {

int rt_scene_light_sampling(rt_ctx* c, int32_t mode) {
  if (!c) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "rt_scene_light_sampling: no scene uploaded");
  if (!known_mode(mode)) return fail(c, RT_E_INVALID, "rt_scene_light_sampling: unknown mode %d", mode);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (like rt_scene_light_pick: a setting changes between passes)
  c->light_sampling = mode;
  return RT_OK;
}

int rt_light_sample_at(rt_ctx* c, int32_t n, const double* points, const double* normals, uint64_t seed,
                       rt_light_sample* out) {
  if (!c) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "rt_light_sample_at: no scene uploaded");
  if (c->light_list.empty()) return fail(c, RT_E_INVALID, "rt_light_sample_at: the scene lists no light");
  if (n < 0 || (n > 0 && (!points || !normals || !out))) return fail(c, RT_E_INVALID, "bad vertex batch");
  if (n == 0) return RT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  // one buffer: points [n][3], normals [n][3], then the records [n]
  DevBuf b;
  const size_t nd = (size_t)n;
  int st = ensure(c, b, nd * 6 * sizeof(double) + nd * sizeof(rt_light_sample));
  if (!st) {
    double* dp = static_cast<double*>(b.p);
    double* dn = dp + nd * 3;
    rt_light_sample* dout = reinterpret_cast<rt_light_sample*>(dn + nd * 3);
    hipError_t e = hipMemcpyAsync(dp, points, nd * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dn, normals, nd * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
      e = launch_light_sample(static_cast<const DLight*>(c->lights.p), (int)c->light_list.size(), pass_light_grid(c),
                              pass_light_sample(c), seed, n, dp, dn, dout, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, nd * sizeof(rt_light_sample), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) st = fail(c, RT_E_HIP, "rt_light_sample_at: %s", hipGetErrorString(e));
  }
  release(b);
  return st;
}

int rt_light_sample_host(const rt_scene_desc* d, int32_t cells, int32_t mode, int32_t n, const double* points,
                         const double* normals, uint64_t seed, rt_light_sample* out) {
  if (!d || validate(d, nullptr) || !known_mode(mode) || cells < 0 || cells > kLightGridMaxCells) return RT_E_INVALID;
  if (n < 0 || (n > 0 && (!points || !normals || !out))) return RT_E_INVALID;
  const LightList l = list_lights(d);
  if (l.dev.empty()) return RT_E_INVALID;
  LightGridTable t;
  if (cells > 0 && build_light_grid(l, cells, true, &t)) return RT_E_INVALID;
  for (int32_t i = 0; i < n; ++i)
    host_light_sample(l.dev, cells > 0 ? &t : nullptr, mode, seed, (uint32_t)i,
                      points + (size_t)i * 3, normals + (size_t)i * 3, out + i);
  return RT_OK;
}

}  // extern "C"
