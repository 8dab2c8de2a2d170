// rt_light_pick.cpp — the spatially weighted light pick of include/shirley_rt.h (added within ABI 11;
// scene_compile.cpp build_light_grid, light_pick.h, direct.hip's light_pick_kernel).
#include "rt_ctx.h"

using namespace rt;

extern "C" {

int rt_light_grid_host(const rt_scene_desc* d, int32_t cells, rt_light_grid* info, double* cdf) {
  if (!d || !info || validate(d, nullptr)) return RT_E_INVALID;
  LightGridTable t;
  const int st = build_light_grid(list_lights(d), cells, cdf != nullptr, &t);
  if (st) return st;
  *info = t.info;
  for (size_t i = 0; i < t.cdf.size(); ++i) cdf[i] = t.cdf[i];
  return RT_OK;
}

int rt_scene_light_pick(rt_ctx* c, int32_t cells, rt_light_grid* info) {
  if (!c) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "rt_scene_light_pick: no scene uploaded");
  if (cells < 0 || cells > kLightGridMaxCells)
    return fail(c, RT_E_INVALID, "rt_scene_light_pick: cells %d outside 0 ... %d", cells, kLightGridMaxCells);
  LightGridTable t;
  if (cells > 0) {
    LightList l;
    l.dev = c->light_dev;
    if (build_light_grid(l, cells, true, &t))
      return fail(c, RT_E_INVALID, "rt_scene_light_pick: a grid of %d cells for %zu lights has more than 2^22 entries",
                  cells, l.dev.size());
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (queued passes may still read the rows this call replaces)
  DLightGrid g{};
  if (!t.cdf.empty()) {
    const int st = upload(c, c->light_cdf, t.cdf.data(), t.cdf.size() * sizeof(double));
    if (st) return st;
    g.cdf = static_cast<const double*>(c->light_cdf.p);
    for (int a = 0; a < 3; ++a) {
      g.lo[a] = t.info.lo[a];
      g.inv[a] = t.info.n[a] == 1 ? 0.0 : (double)t.info.n[a] / (t.info.hi[a] - t.info.lo[a]);
      g.n[a] = t.info.n[a];
    }
  } else {
    release(c->light_cdf);
  }
  c->light_grid = g;
  c->light_grid_info = t.info;
  c->light_cells = cells;
  c->light_vis = rt_light_visibility{};  // the new rows are the plain grid's (rt_scene_light_visibility: off)
  c->light_vis_masks.clear();
  if (info) *info = t.info;
  return RT_OK;
}

int rt_light_pick_at(rt_ctx* c, int32_t n, const double* points, const double* xi, int32_t* light, double* prob) {
  if (!c) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "rt_light_pick_at: no scene uploaded");
  const DLightGrid* g = pass_light_grid(c);
  if (!g) return fail(c, RT_E_INVALID, "rt_light_pick_at: no light grid is set (rt_scene_light_pick), or no light");
  if (n < 0 || (n > 0 && (!points || !xi || !light || !prob))) return fail(c, RT_E_INVALID, "bad point batch");
  if (n == 0) return RT_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  // one buffer: points [n][3], xi [n], prob [n], then light [n]
  DevBuf b;
  const size_t nd = (size_t)n;
  int st = ensure(c, b, nd * 5 * sizeof(double) + nd * sizeof(int32_t));
  if (!st) {
    double* dp = static_cast<double*>(b.p);
    double* dxi = dp + nd * 3;
    double* dprob = dxi + nd;
    int32_t* dlight = reinterpret_cast<int32_t*>(dprob + nd);
    hipError_t e = hipMemcpyAsync(dp, points, nd * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dxi, xi, nd * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
      e = launch_light_pick(*g, (int)c->light_list.size(), n, dp, dxi, dlight, dprob, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(prob, dprob, nd * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(light, dlight, nd * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) st = fail(c, RT_E_HIP, "rt_light_pick_at: %s", hipGetErrorString(e));
  }
  release(b);
  return st;
}

}  // extern "C"
