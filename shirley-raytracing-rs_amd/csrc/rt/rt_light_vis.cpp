// rt_light_vis.cpp — the visibility-aware light pick of include/shirley_rt.h (added within ABI 11; lightvis.hip,
// scene_compile.cpp build_light_grid / light_visibility_ray): the scene setting, the masks it
// traced, and the rays and the rows in plain C++ without a device.
#include "lightvis.h"
#include "rt_ctx.h"

using namespace rt;

namespace {

// What both host functions check first: the scene, the grid and the ray count.
int host_grid(const rt_scene_desc* d, int32_t cells, int32_t rays, LightList* l, LightGridTable* t) {
  if (!d || validate(d, nullptr) || !light_visibility_rays_ok(rays)) return RT_E_INVALID;
  *l = list_lights(d);
  if (l->dev.empty() || build_light_grid(*l, cells, false, t)) return RT_E_INVALID;
  return RT_OK;
}

// Uploads rows in the place of the grid's (the table's shape does not change).
int put_rows(rt_ctx* c, const LightGridTable& t) {
  const int st = upload(c, c->light_cdf, t.cdf.data(), t.cdf.size() * sizeof(double));
  if (st) return st;
  c->light_grid.cdf = static_cast<const double*>(c->light_cdf.p);
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_light_visibility_rays_host(const rt_scene_desc* d, int32_t cells, int32_t rays, uint64_t seed, int32_t cell,
                                  int32_t light, double* rays_out, uint8_t* traced) {
  LightList l;
  LightGridTable t;
  if (host_grid(d, cells, rays, &l, &t) || !rays_out || !traced) return RT_E_INVALID;
  const rt_light_grid& g = t.info;
  if (cell < 0 || cell >= g.n[0] * g.n[1] * g.n[2] || light < 0 || light >= g.n_lights) return RT_E_INVALID;
  for (int32_t i = 0; i < rays; ++i)
    traced[i] = light_visibility_ray(g, l.dev[(size_t)light], seed, (uint32_t)cell, (uint32_t)light, (uint32_t)i,
                                     rays_out + (size_t)i * 6, rays_out + (size_t)i * 6 + 3)
                    ? 1
                    : 0;
  return RT_OK;
}

int rt_light_visibility_rows_host(const rt_scene_desc* d, int32_t cells, int32_t rays, const uint32_t* masks,
                                  double* cdf) {
  LightList l;
  LightGridTable t;
  if (host_grid(d, cells, rays, &l, &t) || !masks || !cdf) return RT_E_INVALID;
  const int st = build_light_grid(l, cells, true, &t, masks, rays);
  if (st) return st;
  for (size_t i = 0; i < t.cdf.size(); ++i) cdf[i] = t.cdf[i];
  return RT_OK;
}

int rt_scene_light_visibility(rt_ctx* c, int32_t rays, uint64_t seed, rt_light_visibility* report) {
  if (!c) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "rt_scene_light_visibility: no scene uploaded");
  if (rays != 0 && !light_visibility_rays_ok(rays))
    return fail(c, RT_E_INVALID, "rt_scene_light_visibility: rays %d is not 0, 1, 2, 4, 8, 16 or 32", rays);
  LightList l;
  l.dev = c->light_dev;
  LightGridTable t;
  if (rays == 0) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (queued passes may still read the rows this call replaces)
    if (c->light_vis.rays) {  // the plain rows again
      if (build_light_grid(l, c->light_cells, true, &t)) return fail(c, RT_E_INVALID, "rt_scene_light_visibility: no grid");
      const int st = put_rows(c, t);
      if (st) return st;
    }
    c->light_vis = rt_light_visibility{};
    c->light_vis_masks.clear();
    if (report) *report = c->light_vis;
    return RT_OK;
  }
  if (c->scene.exts)
    return fail(c, RT_E_UNSUPPORTED, "rt_scene_light_visibility: scenes with book-2 objects are not supported");
  if (c->light_cells < 1)
    return fail(c, RT_E_INVALID, "rt_scene_light_visibility: no light grid is set (rt_scene_light_pick)");
  if (c->light_list.empty()) return fail(c, RT_E_INVALID, "rt_scene_light_visibility: the scene lists no light");
  const rt_light_grid& g = c->light_grid_info;
  const size_t L = (size_t)g.n_lights;
  const size_t n_cells = (size_t)g.n[0] * (size_t)g.n[1] * (size_t)g.n[2];
  const size_t pairs = n_cells * L;  // <= 2^22: rt_scene_light_pick refused a larger table
  const size_t waves = (pairs * (size_t)rays + kWave - 1) / kWave;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int st = ensure(c, c->light_vis_out, (pairs + waves) * sizeof(uint32_t));
  if (st) return st;
  uint32_t* masks_dev = static_cast<uint32_t*>(c->light_vis_out.p);
  DLightVisCells Z;
  for (int a = 0; a < 3; ++a) Z.size[a] = (g.hi[a] - g.lo[a]) / (double)g.n[a];
  // 1. the kernel, between two events
  hipEvent_t ev[2] = {nullptr, nullptr};
  std::vector<uint32_t> out(pairs + waves);
  float ms = 0.0f;
  hipError_t e = hipEventCreate(&ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&ev[1]);
  if (e == hipSuccess) e = hipEventRecord(ev[0], c->stream);
  if (e == hipSuccess)
    e = launch_lightvis(c->scene, c->place.wide, static_cast<const DLight*>(c->lights.p), (int)L, c->light_grid, Z,
                        seed, rays, (uint32_t)pairs, masks_dev, masks_dev + pairs, c->stream);
  if (e == hipSuccess) e = hipEventRecord(ev[1], c->stream);
  // 2. the masks and the waves' counts back
  if (e == hipSuccess)
    e = hipMemcpyAsync(out.data(), masks_dev, out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  if (e != hipSuccess) return fail(c, RT_E_HIP, "rt_scene_light_visibility: %s", hipGetErrorString(e));
  // 3. the rows, on the host
  if ((st = build_light_grid(l, c->light_cells, true, &t, out.data(), rays)))
    return fail(c, st, "rt_scene_light_visibility: the grid's build failed");
  // 4. ... in place of the grid's
  if ((st = put_rows(c, t))) return st;
  rt_light_visibility r{};
  r.rays = rays;
  r.seed = seed;
  r.pairs = pairs;
  r.kernel_ms = (double)ms;
  for (size_t w = 0; w < waves; ++w) r.traced += out[pairs + w];
  for (size_t cell = 0; cell < n_cells; ++cell) {
    uint32_t valid = 0;
    for (size_t j = 0; j < L; ++j) {
      valid |= out[cell * L + j];
      r.unoccluded += (uint64_t)__builtin_popcount(out[cell * L + j]);
    }
    r.dead_points += (uint64_t)(rays - __builtin_popcount(valid));
  }
  out.resize(pairs);
  c->light_vis_masks = std::move(out);
  c->light_vis = r;
  if (report) *report = r;
  return RT_OK;
}

int rt_light_visibility_masks(rt_ctx* c, uint32_t* masks) {
  if (!c) return RT_E_INVALID;
  if (!c->have_scene) return fail(c, RT_E_INVALID, "rt_light_visibility_masks: no scene uploaded");
  if (!c->light_vis.rays) return fail(c, RT_E_INVALID, "rt_light_visibility_masks: the setting is off");
  if (!masks) return fail(c, RT_E_INVALID, "rt_light_visibility_masks: the buffer is NULL");
  for (size_t i = 0; i < c->light_vis_masks.size(); ++i) masks[i] = c->light_vis_masks[i];
  return RT_OK;
}

}  // extern "C"
