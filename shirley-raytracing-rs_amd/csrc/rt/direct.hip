// direct.hip — rt_render_direct: per-pixel sums of the feature vertex's emission and of a one-light-sample
// estimate of its direct illumination from the scene's light list (include/shirley_rt.h).
//
// direct_kernel is a tile pass (one wave per 8x8 tile, one lane per pixel, the sample loop inside the lane, the
// camera ray and the dielectric chain to the feature vertex, the wave's marble for a Perlin albedo, so lanes of
// an edge tile outside the image stay, idle, for that wave-wide step) that, at a Lambertian or FairyLight vertex,
// calls direct_light (direct.h), whose shadow ray asks the any-hit walk occluded4 (occlusion.h).  The light table
// is a kernel argument of its own, and so is the light grid of a kPickGrid instance (light_pick.h, DESIGN.md §18;
// the last argument, an empty record in the uniform instances).  No atomics, no inter-wave traffic.  Its block
// size and launch are the frame's (pass_frame.h); the kernel spells the frame's device pieces out, because with
// any of them it runs 0.5 % slower on the night frame (profiles/passframe/direct_pieces.json).
// Reference scenes only (no book-2 records): EXT = false instances.
// A kSampleCone instance (light_cone.h) samples sphere lights by solid angle, a kSampleAll instance
// (light_rect.h) rect lights too.
// light_pick_kernel (rt_light_pick_at) runs the grid's pick alone, one point per lane; light_sample_kernel
// (rt_light_sample_at) the whole light sample but its shadow ray.
#include <hip/hip_runtime.h>

#include "direct.h"
#include "pass_frame.h"
#include "rt_launch.h"

namespace rt {

template <int THREADS, int MODE, int PICK, int SAMPLE>
__global__ __launch_bounds__(THREADS) void direct_kernel(DScene S, DCamera C, uint64_t seed, int s_begin, int s_end,
                                                         int chain, int tiles_x, int n_tiles,
                                                         const DLight* __restrict__ lights, int n_lights,
                                                         double* __restrict__ emission,
                                                         double* __restrict__ direct,
                                                         const typename PickGrid<PICK>::type grid) {
  extern __shared__ unsigned char lds_raw[];
  const int tid = threadIdx.x;
  typedef DNode4F N4;
  N4* lds_nodes = reinterpret_cast<N4*>(lds_raw);
  DPrim* lds_prims = reinterpret_cast<DPrim*>(lds_raw + (size_t)S.n_lds_nodes4 * sizeof(N4));
  const DPerlin* lds_perlin = (MODE == kSceneLds && S.n_lds_perlin > 0)
                                  ? reinterpret_cast<const DPerlin*>(lds_prims + S.n_lds_prims)
                                  : nullptr;
  unsigned char* stk_base = lds_raw + (size_t)S.n_lds_nodes4 * sizeof(N4) +
                            (MODE == kSceneLds ? (size_t)S.n_lds_prims * sizeof(DPrim) +
                                                     (size_t)S.n_lds_perlin * sizeof(DPerlin) +
                                                     (size_t)S.n_lds_mats * sizeof(DMat) +
                                                     (size_t)S.n_lds_texs * sizeof(DTex)
                                               : 0);
  unsigned* stk = reinterpret_cast<unsigned*>(stk_base) + tid;
  stage_nodes4<MODE>(S, lds_nodes, lds_prims);
  // wave w of the block renders tile blockIdx * (THREADS / 64) + w; lane l its pixel (l % 8, l / 8)
  const int tile = blockIdx.x * (THREADS / kWave) + tid / kWave;
  const int lane = tid % kWave;
  const int px = (tile % tiles_x) * kTile + lane % kTile;
  const int py = (tile / tiles_x) * kTile + lane / kTile;
  // (a whole wave past the last tile leaves together; lanes of an edge tile outside the image stay, idle,
  // for the wave-wide marble)
  if (tile >= n_tiles) return;
  const bool active = px < C.width && py < C.height;
  const uint32_t pix = (uint32_t)py * (uint32_t)C.width + (uint32_t)px;
  v3 se = V(0.0, 0.0, 0.0), sd = V(0.0, 0.0, 0.0);
  unsigned visits = 0, ptests = 0;
#ifdef RT_PHASE_TIMING
  unsigned long long steps = 0;
#endif
  for (int s = s_begin; s < s_end; ++s) {  // wave-uniform
    Rng rng{pix, (uint32_t)s, 0u, 0u, 0u};
    v3 o = V(0.0, 0.0, 0.0), d = V(1.0, 1.0, 1.0);
    bool hit = false, need_pn = false;
    int prim = -1, face = -1, leaf = -1, mat = 0, ptab = 0, mk = -1;
    double psc = 0.0;
    Hit h;
    h.point = V(0.0, 0.0, 0.0);
    h.normal = h.point;
    h.t = h.u = h.v = 0.0;
    h.front_face = false;
    if (active) {
      const double jx = (double)px + rng_next(rng, seed);  // render.rs:60-63
      const double jy = (double)py + rng_next(rng, seed);
      camera_ray(C, rng, seed, jx, jy, o, d);
      int left = chain;
      for (;;) {  // through at most `chain` dielectric vertices; each kernel keeps this loop
        double t_best = __builtin_inf();
        face = -1;
        prim = traverse4<THREADS, MODE, false>(S, lds_nodes, lds_prims, o, d, 0.001, t_best, face, stk, rng, seed,
                                                    visits, ptests RT_STAT_ARG(steps));
        hit = prim >= 0;
        if (!hit) break;
        const DPrim pr = (MODE == kSceneLds) ? lds_prims[prim] : S.prims[prim];
        hit_record<false, false>(S, pr, face, o, d, t_best, rng, seed, h);
        mat = pr.material;
        mk = S.mats[mat].kind;
        if (mk != RT_MAT_DIELECTRIC || left <= 0) break;
        --left;
        const v3 rs = draw_diel(rng, seed);
        shade_dielectric(S.mats[mat], rs, unit_fast(d), rng, o, d, h);
      }
      if (hit && (mk == RT_MAT_LAMBERTIAN || mk == RT_MAT_FAIRY_LIGHT || mk == RT_MAT_DIFFUSE_LIGHT)) {
        leaf = resolve_texture(S, S.mats[mat].tex, h.point);
        const DTex& tx = S.texs[leaf];
        if (tx.kind == RT_TEX_PERLIN) {
          need_pn = true;
          ptab = tx.table;
          psc = tx.scale;
        }
      }
    }
    // the wave's marble values (wave-uniform: every lane of the wave is here)
    const double pn = lds_perlin ? marble_coop((LdsPerlin*)lds_perlin, need_pn, ptab, psc, h.point)
                                 : marble_coop(S.perlin, need_pn, ptab, psc, h.point);
    if (active) {
      v3 em = V(0.0, 0.0, 0.0), dl = V(0.0, 0.0, 0.0);
      if (!hit) {
        em = sky_unit(S, unit_fast(d));
      } else if (leaf >= 0) {
        v3 a = leaf_texture_value(S, S.texs, leaf, pn, prim, face, h);
        if (mk == RT_MAT_DIFFUSE_LIGHT) {  // lighting.rs:21-29: emits, never scatters
          em = a;
        } else {
          if (mk == RT_MAT_FAIRY_LIGHT) {  // shade_factor's emission and attenuation (lighting.rs:42-66)
            const double sc = dot(h.normal, scale(d, -1.0));
            em = scale(a, sc / len(d));
            a = unit(a);
          }
          if (n_lights > 0)
            dl = direct_light<THREADS, MODE, PICK, SAMPLE>(S, lds_nodes, lds_prims, lights, n_lights, rng, seed,
                                                           h.point, h.normal, a, stk, visits, ptests, grid);
        }
      }
      se = se + em;
      sd = sd + dl;
    }
  }
  if (!active) return;
  const size_t p = (size_t)py * (size_t)C.width + (size_t)px;
  if (emission) {
    emission[p * 3 + 0] = se.x;
    emission[p * 3 + 1] = se.y;
    emission[p * 3 + 2] = se.z;
  }
  if (direct) {
    direct[p * 3 + 0] = sd.x;
    direct[p * 3 + 1] = sd.y;
    direct[p * 3 + 2] = sd.z;
  }
}

// rt_render_direct
// rt_render_direct; `grid` (null: the uniform pick) is read only where n_lights > 0; `sample`: kSampleArea,
// kSampleCone or kSampleAll, the instances' sample kind
hipError_t launch_direct(const DScene& S, bool wide, const DCamera& C, uint64_t seed, int s_begin, int s_end, int chain,
                         const DLight* lights, int n_lights, const DLightGrid* grid, int sample, double* emission,
                         double* direct, hipStream_t stream) {
  if (S.exts) return hipErrorInvalidValue;  // (the caller refuses book-2 scenes)
  if (n_lights > 0 && !lights) return hipErrorInvalidValue;
  if (grid && n_lights > 0 && !grid->cdf) return hipErrorInvalidValue;
  const TileGrid G = tile_grid(C);
  return dispatch_placement<kPassThreadsWide>(S, wide, [&](auto threads, auto mode) {
    constexpr int T = decltype(threads)::value, M = decltype(mode)::value;
    auto go = [&](auto kernel, auto g) {
      return launch_block(kernel, G.blocks(T), T, block_lds_bytes<M>(S, node4_bytes(false), T), stream, S, C, seed,
                          s_begin, s_end, chain, G.tiles_x, G.n_tiles, lights, n_lights, emission, direct, g);
    };
    if (sample == kSampleAll)
      return grid && n_lights > 0 ? go(direct_kernel<T, M, kPickGrid, kSampleAll>, *grid)
                                  : go(direct_kernel<T, M, kPickUniform, kSampleAll>, NoLightGrid{});
    if (sample == kSampleCone)
      return grid && n_lights > 0 ? go(direct_kernel<T, M, kPickGrid, kSampleCone>, *grid)
                                  : go(direct_kernel<T, M, kPickUniform, kSampleCone>, NoLightGrid{});
    return grid && n_lights > 0 ? go(direct_kernel<T, M, kPickGrid, kSampleArea>, *grid)
                                : go(direct_kernel<T, M, kPickUniform, kSampleArea>, NoLightGrid{});
  });
}

// rt_light_pick_at: a ray-batch-style kernel (one point per lane, a kHitThreads block) that runs only the pick.
__global__ __launch_bounds__(kHitThreads) void light_pick_kernel(const DLightGrid grid, int n_lights, int n,
                                                                 const double* __restrict__ points,
                                                                 const double* __restrict__ xi,
                                                                 int32_t* __restrict__ light,
                                                                 double* __restrict__ prob) {
  const int i = blockIdx.x * kHitThreads + (int)threadIdx.x;
  if (i >= n) return;
  const double* p = points + (size_t)i * 3;
  const int cell = light_cell(grid, p[0], p[1], p[2]);
  double pk;
  light[i] = light_pick(grid, cell, n_lights, xi[i], pk);
  prob[i] = pk;
}

hipError_t launch_light_pick(const DLightGrid& grid, int n_lights, int n, const double* points, const double* xi,
                             int32_t* light, double* prob, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (n_lights < 1 || !grid.cdf || !points || !xi || !light || !prob) return hipErrorInvalidValue;
  return launch_block(light_pick_kernel, (n + kHitThreads - 1) / kHitThreads, kHitThreads, 0, stream, grid, n_lights, n,
                      points, xi, light, prob);
}

// rt_light_sample_at: one vertex per lane on the path key (seed, pixel = i, sample 0) from draw 0 — the whole
// light sample but its shadow ray (light_sample_point, then both forms of light_sample_g).
template <int PICK, int SAMPLE>
__global__ __launch_bounds__(kHitThreads) void light_sample_kernel(const DLight* __restrict__ lights, int n_lights,
                                                                   uint64_t seed, int n,
                                                                   const double* __restrict__ points,
                                                                   const double* __restrict__ normals,
                                                                   rt_light_sample* __restrict__ out,
                                                                   const typename PickGrid<PICK>::type grid) {
  const int i = blockIdx.x * kHitThreads + (int)threadIdx.x;
  if (i >= n) return;
  const double* p = points + (size_t)i * 3;
  const double* q = normals + (size_t)i * 3;
  Rng rng{(uint32_t)i, 0u, 0u, 0u, 0u};
  int cell = 0;
  const LightSample s =
      light_sample_point<PICK, SAMPLE>(lights, n_lights, rng, seed, V(p[0], p[1], p[2]), V(q[0], q[1], q[2]), grid, cell);
  rt_light_sample r;
  r.light = s.li;
  r.flags = s.flags;
  r.draws = rng.draw;
  r.pad = 0;
  r.w[0] = s.w.x;
  r.w[1] = s.w.y;
  r.w[2] = s.w.z;
  r.cx = s.cx;
  r.cy = s.cy;
  const bool zero = SAMPLE == kSampleAll ? (s.flags & kLightZero) != 0 : s.flags != 0;
  r.g_plain = zero ? 0.0 : light_sample_g<false, PICK, SAMPLE>(lights[s.li], s, (double)n_lights);
  r.g_mis = zero ? 0.0 : light_sample_g<true, PICK, SAMPLE>(lights[s.li], s, (double)n_lights);
  out[i] = r;
}

hipError_t launch_light_sample(const DLight* lights, int n_lights, const DLightGrid* grid, int sample, uint64_t seed,
                               int n, const double* points, const double* normals, rt_light_sample* out,
                               hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (n_lights < 1 || !lights || !points || !normals || !out || (grid && !grid->cdf)) return hipErrorInvalidValue;
  auto go = [&](auto kernel, auto g) {
    return launch_block(kernel, (n + kHitThreads - 1) / kHitThreads, kHitThreads, 0, stream, lights, n_lights, seed, n,
                        points, normals, out, g);
  };
  if (sample == kSampleAll)
    return grid ? go(light_sample_kernel<kPickGrid, kSampleAll>, *grid)
                : go(light_sample_kernel<kPickUniform, kSampleAll>, NoLightGrid{});
  if (sample == kSampleCone)
    return grid ? go(light_sample_kernel<kPickGrid, kSampleCone>, *grid)
                : go(light_sample_kernel<kPickUniform, kSampleCone>, NoLightGrid{});
  return grid ? go(light_sample_kernel<kPickGrid, kSampleArea>, *grid)
              : go(light_sample_kernel<kPickUniform, kSampleArea>, NoLightGrid{});
}

}  // namespace rt
