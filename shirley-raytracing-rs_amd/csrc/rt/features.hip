// features.hip — rt_render_features: per-pixel sums of albedo, normal and depth along each sample's own
// path (include/shirley_rt.h, ABI 10), the guide images of the à-trous filter (denoise.hip).
//
// features_kernel stands in the tile-pass frame (pass_frame.h): one wave per 8x8 tile, one lane per pixel, the
// sample loop inside the lane, the camera ray and the dielectric chain to the feature vertex, the texture leaf
// and the wave's marble, so lanes of an edge tile outside the image stay, idle, for that wave-wide step.
// It takes the block layout, the launch, texture_leaf and wave_marble from the frame and spells out the tile
// mapping and the camera ray itself: through tile_lane / sample_ray the night frame ran 0.3 % slower
// (profiles/passframe/features_pieces.json).
// Reference scenes only (no book-2 records): EXT = false instances.
#include <hip/hip_runtime.h>

#include "pass_frame.h"
#include "rt_launch.h"

namespace rt {

template <int THREADS, int MODE>
__global__ __launch_bounds__(THREADS) void features_kernel(DScene S, DCamera C, uint64_t seed, int s_begin,
                                                               int s_end, int chain, int tiles_x, int n_tiles,
                                                               double* __restrict__ albedo,
                                                               double* __restrict__ normal,
                                                               double* __restrict__ depth) {
  extern __shared__ unsigned char lds_raw[];
  const BlockLds<DNode4F> L = carve_block_lds<MODE, DNode4F>(S, lds_raw);
  stage_nodes4<MODE>(S, L.nodes, L.prims);
  // wave w of the block renders tile blockIdx * (THREADS / 64) + w; lane l its pixel (l % 8, l / 8)
  const int tid = threadIdx.x;
  const int tile = blockIdx.x * (THREADS / kWave) + tid / kWave;
  const int lane = tid % kWave;
  const int px = (tile % tiles_x) * kTile + lane % kTile;
  const int py = (tile / tiles_x) * kTile + lane / kTile;
  // (a whole wave past the last tile leaves together; lanes of an edge tile outside the image stay, idle,
  // for the wave-wide marble)
  if (tile >= n_tiles) return;
  const bool active = px < C.width && py < C.height;
  const uint32_t pix = (uint32_t)py * (uint32_t)C.width + (uint32_t)px;
  v3 sa = V(0.0, 0.0, 0.0), sn = V(0.0, 0.0, 0.0);
  double sz = 0.0;
  unsigned visits = 0, ptests = 0;
#ifdef RT_PHASE_TIMING
  unsigned long long steps = 0;
#endif
  for (int s = s_begin; s < s_end; ++s) {  // wave-uniform
    Rng rng{pix, (uint32_t)s, 0u, 0u, 0u};
    v3 o = V(0.0, 0.0, 0.0), d = V(1.0, 1.0, 1.0);
    bool hit = false, need_pn = false;
    int prim = -1, face = -1, leaf = -1, mat = 0, ptab = 0, mk = -1;
    double psc = 0.0, z = 0.0;
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
      for (bool first = true;; first = false) {  // through at most `chain` dielectric vertices
        double t_best = __builtin_inf();
        face = -1;
        prim = traverse4<THREADS, MODE, false>(S, L.nodes, L.prims, o, d, 0.001, t_best, face, L.stk, rng, seed, visits,
                                               ptests RT_STAT_ARG(steps));
        hit = prim >= 0;
        if (first) z = hit ? t_best : 0.0;
        if (!hit) break;
        const DPrim pr = (MODE == kSceneLds) ? L.prims[prim] : S.prims[prim];
        hit_record<false, false>(S, pr, face, o, d, t_best, rng, seed, h);
        mat = pr.material;
        mk = S.mats[mat].kind;
        if (mk != RT_MAT_DIELECTRIC || left <= 0) break;
        // one dielectric vertex: the renderer's segment (shade_factor's dielectric branch)
        --left;
        const v3 rs = draw_diel(rng, seed);
        shade_dielectric(S.mats[mat], rs, unit_fast(d), rng, o, d, h);
      }
      if (hit && (mk == RT_MAT_LAMBERTIAN || mk == RT_MAT_FAIRY_LIGHT || mk == RT_MAT_DIFFUSE_LIGHT))
        leaf = texture_leaf(S, S.mats[mat].tex, h.point, need_pn, ptab, psc);
    }
    // the wave's marble values (wave-uniform: every lane of the wave is here)
    const double pn = wave_marble(S, L.perlin, need_pn, ptab, psc, h.point);
    if (active) {
      v3 a;
      if (!hit) {
        a = sky_unit(S, unit_fast(d));
      } else {
        const DMat& m = S.mats[mat];
        if (mk == RT_MAT_METAL) a = V(m.albedo[0], m.albedo[1], m.albedo[2]);
        else if (leaf >= 0) a = leaf_texture_value(S, S.texs, leaf, pn, prim, face, h);
        else a = V(1.0, 1.0, 1.0);  // a dielectric with the chain exhausted
        sn = sn + h.normal;
      }
      sa = sa + a;
      sz += z;
    }
  }
  if (!active) return;
  const size_t p = (size_t)py * (size_t)C.width + (size_t)px;
  if (albedo) {
    albedo[p * 3 + 0] = sa.x;
    albedo[p * 3 + 1] = sa.y;
    albedo[p * 3 + 2] = sa.z;
  }
  if (normal) {
    normal[p * 3 + 0] = sn.x;
    normal[p * 3 + 1] = sn.y;
    normal[p * 3 + 2] = sn.z;
  }
  if (depth) depth[p] = sz;
}

// rt_render_features
hipError_t launch_features(const DScene& S, bool wide, const DCamera& C, uint64_t seed, int s_begin, int s_end,
                           int chain, double* albedo, double* normal, double* depth, hipStream_t stream) {
  if (S.exts) return hipErrorInvalidValue;  // (the caller refuses book-2 scenes)
  const TileGrid G = tile_grid(C);
  return dispatch_placement<kPassThreadsWide>(S, wide, [&](auto threads, auto mode) {
    constexpr int T = decltype(threads)::value, M = decltype(mode)::value;
    return launch_block(features_kernel<T, M>, G.blocks(T), T, block_lds_bytes<M>(S, node4_bytes(false), T), stream, S,
                        C, seed, s_begin, s_end, chain, G.tiles_x, G.n_tiles, albedo, normal, depth);
  });
}

}  // namespace rt
