// features.hip — rt_render_features: per-pixel sums of albedo, normal and depth along each sample's own
// path (include/shirley_rt.h, ABI 10), the guide images of the à-trous filter (denoise.hip).
//
// Modelled on probe_kernel (trace.hip): the same MODE staging of nodes / primitives / Perlin tables, the
// render traversal traverse4, hit_record, resolve_texture, the wave's marble and the texture leaf value.
// One wave per 8x8 tile, one lane per pixel, the sample loop inside the lane; a sample's camera ray is the
// serial camera_ray on draws 0, 1 (jitter) and the lens-disk draws, as the wavefront and split engines form
// it, and a dielectric vertex of the chain is draw_diel + shade_dielectric, the hop pass's copy of the
// megakernel's dielectric branch.  Reference scenes only (no book-2 records): EXT = false instances.
#include <hip/hip_runtime.h>

#include "rt_device.h"
#include "rt_launch.h"

namespace rt {

// Block of the scene-in-LDS placements (`wide`): the megakernel's 1024 threads, which the placement plan
// sized the LDS stacks for — 16 tiles share one staged copy of the scene.  At 128 VGPRs the kernel spills 4.
// Measured at 16 spp, chain 8 (profiles/denoise/features_block_ab.json): headline 1200x800 3.44 ms against
// 4.49 ms (512 threads) and 6.88 ms (256); Cornell 600x600 0.295 ms against 0.268 / 0.231 ms.
constexpr int kFeatThreadsWide = kTraceThreadsWide;

template <int THREADS, int MODE>
__global__ __launch_bounds__(THREADS) void features_kernel(DScene S, DCamera C, uint64_t seed, int s_begin,
                                                               int s_end, int chain, int tiles_x, int n_tiles,
                                                               double* __restrict__ albedo,
                                                               double* __restrict__ normal,
                                                               double* __restrict__ depth) {
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
      for (bool first = true;; first = false) {
        double t_best = __builtin_inf();
        face = -1;
        prim = traverse4<THREADS, MODE, false>(S, lds_nodes, lds_prims, o, d, 0.001, t_best, face, stk, rng, seed,
                                                    visits, ptests RT_STAT_ARG(steps));
        hit = prim >= 0;
        if (first) z = hit ? t_best : 0.0;
        if (!hit) break;
        const DPrim pr = (MODE == kSceneLds) ? lds_prims[prim] : S.prims[prim];
        hit_record<false, false>(S, pr, face, o, d, t_best, rng, seed, h);
        mat = pr.material;
        mk = S.mats[mat].kind;
        if (mk != RT_MAT_DIELECTRIC || left <= 0) break;
        // one dielectric vertex: the renderer's segment (shade_factor's dielectric branch)
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

template <int THREADS, int MODE>
static hipError_t launch_features_1(const DScene& S, const DCamera& C, uint64_t seed, int s_begin, int s_end, int chain,
                                    double* albedo, double* normal, double* depth, hipStream_t stream) {
  const int tiles_x = (C.width + kTile - 1) / kTile, tiles_y = (C.height + kTile - 1) / kTile;
  const int n_tiles = tiles_x * tiles_y;
  const int per_block = THREADS / kWave;
  const int blocks = (n_tiles + per_block - 1) / per_block;
  const size_t lds = trace_lds_bytes(S.n_lds_nodes4, node4_bytes(false), MODE == kSceneLds ? S.n_lds_prims : 0,
                                     MODE == kSceneLds ? S.n_lds_perlin : 0, S.stack_depth4, THREADS,
                                     MODE == kSceneLds ? S.n_lds_mats : 0, MODE == kSceneLds ? S.n_lds_texs : 0);
  hipError_t e = hipFuncSetAttribute((const void*)features_kernel<THREADS, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((features_kernel<THREADS, MODE>), dim3(blocks), dim3(THREADS), lds, stream, S, C, seed, s_begin, s_end,
                     chain, tiles_x, n_tiles, albedo, normal, depth);
  return hipGetLastError();
}

// rt_render_features: the node / primitive placement the trace kernel uses (`wide`, as launch_probe)
hipError_t launch_features(const DScene& S, bool wide, const DCamera& C, uint64_t seed, int s_begin, int s_end,
                           int chain, double* albedo, double* normal, double* depth, hipStream_t stream) {
  if (S.exts) return hipErrorInvalidValue;  // (the caller refuses book-2 scenes)
  if (wide) {
    if (S.n_lds_prims > 0)
      return launch_features_1<kFeatThreadsWide, kSceneLds>(S, C, seed, s_begin, s_end, chain, albedo, normal, depth, stream);
    return launch_features_1<kFeatThreadsWide, kNodesLds>(S, C, seed, s_begin, s_end, chain, albedo, normal, depth, stream);
  }
  const int mode = S.n_lds_nodes4 >= S.n_nodes4 ? kNodesLds : (S.n_lds_nodes4 == 0 ? kNodesGlobal : kNodesMixed);
  switch (mode) {
    case kNodesLds: return launch_features_1<kHitThreads, kNodesLds>(S, C, seed, s_begin, s_end, chain, albedo, normal, depth, stream);
    case kNodesGlobal: return launch_features_1<kHitThreads, kNodesGlobal>(S, C, seed, s_begin, s_end, chain, albedo, normal, depth, stream);
    default: return launch_features_1<kHitThreads, kNodesMixed>(S, C, seed, s_begin, s_end, chain, albedo, normal, depth, stream);
  }
}

}  // namespace rt
