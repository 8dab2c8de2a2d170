// nee.hip — rt_render_nee: a path integrator that takes one light sample at every Lambertian / FairyLight
// vertex and weights the emission its scatter then lands on (include/shirley_rt.h).
//
// nee_kernel keeps direct_kernel's frame (direct.hip: one wave per 8x8 tile, one lane per pixel, the same LDS
// layout and placements, EXT = false) and runs whole paths in it by lane-level path regeneration: one
// wave-uniform loop whose iteration traces one segment per live lane with probe_kernel's body (trace.hip:
// traverse4, hit_record, the wave's marble_coop and draws_coop, shade_factor — the megakernel's device
// functions on the megakernel's draws), then applies the weight ws to the segment's emission and calls
// direct_light (direct.h) in the lanes whose vertex takes a light sample.  A lane whose path ended adds its
// radiance to its running pixel sum and starts its next sample in the next iteration, so a pixel's samples are
// added in order with no atomics and no inter-wave traffic.  Lanes outside the image and lanes out of samples
// stay in the loop, idle, for the wave-wide steps; the loop ends when the wave's last lane is done, and at the
// latest after (s_end - s_begin) * max_depth iterations — one segment per live lane per iteration cannot
// take more.  The light table and the primitive -> light table are kernel arguments of their own.
#include <hip/hip_runtime.h>

#include "direct.h"
#include "rt_launch.h"

namespace rt {

constexpr int kNeeThreadsWide = kTraceThreadsWide;

template <int THREADS, int MODE, bool MIS>
__global__ __launch_bounds__(THREADS) void nee_kernel(DScene S, DCamera C, uint64_t seed, int s_begin, int s_end,
                                                      int max_depth, int tiles_x, int n_tiles,
                                                      const DLight* __restrict__ lights, int n_lights,
                                                      const int32_t* __restrict__ prim_light,
                                                      double* __restrict__ accum) {
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
  if (tile >= n_tiles) return;  // (a whole wave past the last tile leaves together)
  const bool active = px < C.width && py < C.height;
  const uint32_t pix = (uint32_t)py * (uint32_t)C.width + (uint32_t)px;
  unsigned visits = 0, ptests = 0;
#ifdef RT_PHASE_TIMING
  unsigned long long steps = 0;
#endif
  // the lane's path: sample s, segment k, ray (o, d), attenuation, radiance; prev / cx_prev: the last vertex
  // took a light sample, and the cosine of its scatter direction there
  int s = s_begin, k = 1;
  bool fresh = true, prev = false;
  double cx_prev = 0.0;
  Rng rng{pix, (uint32_t)s_begin, 0u, 0u, 0u};
  v3 o = V(0.0, 0.0, 0.0), d = V(1.0, 1.0, 1.0);
  v3 att = V(1.0, 1.0, 1.0), rad = V(0.0, 0.0, 0.0), sum = V(0.0, 0.0, 0.0);
  // one segment per live lane per iteration: no lane has more than `trips` of them (wave-uniform bound)
  const unsigned long long trips =
      (unsigned long long)(s_end > s_begin ? s_end - s_begin : 0) * (unsigned long long)(max_depth > 0 ? max_depth : 0);
  for (unsigned long long it = 0; it < trips; ++it) {
    const bool live = active && s < s_end;
    if (__ballot(live) == 0ull) break;  // wave-uniform: the wave's last lane is done
    if (live && fresh) {  // the next sample's camera ray (render.rs:60-63)
      rng = Rng{pix, (uint32_t)s, 0u, 0u, 0u};
      const double jx = (double)px + rng_next(rng, seed);
      const double jy = (double)py + rng_next(rng, seed);
      camera_ray(C, rng, seed, jx, jy, o, d);
      att = V(1.0, 1.0, 1.0);
      rad = V(0.0, 0.0, 0.0);
      k = 1;
      prev = false;
      fresh = false;
    }
    // probe_kernel's step 1: closest hit, record, material, texture leaf
    bool hit = false, need_pn = false, need_r = false;
    int prim = -1, face = -1, leaf = -1, mat = 0, ptab = 0, mk = -1;
    double t_best = __builtin_inf(), psc = 0.0;
    Hit h;
    h.point = V(0.0, 0.0, 0.0);
    h.normal = h.point;
    h.t = h.u = h.v = 0.0;
    h.front_face = false;
    if (live) {
      prim = traverse4<THREADS, MODE, false>(S, lds_nodes, lds_prims, o, d, 0.001, t_best, face, stk, rng, seed, visits,
                                             ptests RT_STAT_ARG(steps));
      if (prim >= 0) {
        hit = true;
        const DPrim pr = (MODE == kSceneLds) ? lds_prims[prim] : S.prims[prim];
        hit_record<false, false>(S, pr, face, o, d, t_best, rng, seed, h);
        mat = pr.material;
        mk = S.mats[mat].kind;
        need_r = mk == RT_MAT_LAMBERTIAN || mk == RT_MAT_METAL || mk == RT_MAT_FAIRY_LIGHT || mk == RT_MAT_ISOTROPIC;
        if (mk == RT_MAT_LAMBERTIAN || mk == RT_MAT_FAIRY_LIGHT || mk == RT_MAT_DIFFUSE_LIGHT || mk == RT_MAT_ISOTROPIC) {
          leaf = resolve_texture(S, S.mats[mat].tex, h.point);
          const DTex& tx = S.texs[leaf];
          if (tx.kind == RT_TEX_PERLIN) {
            need_pn = true;
            ptab = tx.table;
            psc = tx.scale;
          }
        }
      }
    }
    const bool ends = live && (!hit || mk == RT_MAT_DIFFUSE_LIGHT);
    // step 3: the wave's marble values and draws (every lane of the wave is here)
    const double pn = lds_perlin ? marble_coop((LdsPerlin*)lds_perlin, need_pn, ptab, psc, h.point)
                                 : marble_coop(S.perlin, need_pn, ptab, psc, h.point);
    const bool scat = live && !ends;
    const int dk = (scat && need_r) ? kDrawSphere : (scat && mk == RT_MAT_DIELECTRIC) ? kDrawDiel : kDrawNone;
    double jx0 = 0.0, jy0 = 0.0;
    const v3 rs = draws_coop(rng, seed, dk, false, 0u, jx0, jy0);
    const v3 un = unit_fast(!live ? V(1.0, 1.0, 1.0) : (scat && need_r && mk != RT_MAT_METAL) ? rs : d);
    // step 4: emitted + scatter, or the sky; then the weight and the light sample
    if (live) {
      bool done = false;
      if (!hit) {
        rad = rad + hmul(att, sky_unit(S, un));  // a sky is never listed
        done = true;
      } else {
        const v3 din = d;  // the segment's direction (shade_factor replaces the ray)
        bool has_emit = false;
        v3 mul = V(1.0, 1.0, 1.0), emit = V(0.0, 0.0, 0.0);
        const bool alive = shade_factor(S, S.texs, S.mats[mat], leaf, pn, rs, un, rng, o, d, h, prim, face, mul, emit,
                                        has_emit);
        if (has_emit) {
          double ws = 1.0;
          const int lj = prev ? prim_light[prim] : -1;
          if (lj >= 0 && (lights[lj].geometry != RT_GEOM_SPHERE || h.front_face)) {
            if (MIS) {
              const double ld2 = (din.x * din.x + din.y * din.y) + din.z * din.z;
              const double ld = sqrt_rn(ld2);
              const double cy = -dot(h.normal, din) / ld;
              const double d2 = (h.t * h.t) * ld2;
              if (cx_prev > 0.0 && cy > 0.0) {
                const double gs = ((cx_prev * cy) / d2) / kDirectPi;
                const double pl = 1.0 / (lights[lj].area * (double)n_lights);
                ws = gs / (pl + gs);
              }
            } else {
              ws = 0.0;
            }
          }
          rad = rad + scale(hmul(att, emit), ws);
        }
        if (!alive) {
          done = true;
        } else {
          prev = false;
          if ((mk == RT_MAT_LAMBERTIAN || mk == RT_MAT_FAIRY_LIGHT) && n_lights > 0 && k < max_depth) {
            // on the path's draws after the scatter's own; stands for segment k + 1's emission
            const v3 dl = direct_light<THREADS, MODE, MIS>(S, lds_nodes, lds_prims, lights, n_lights, rng, seed, h.point,
                                                           h.normal, mul, stk, visits, ptests, prev);
            rad = rad + hmul(att, dl);
            cx_prev = dot(h.normal, d) / sqrt_rn(len2(d));
          }
          att = hmul(att, mul);
          ++k;
          done = k > max_depth;
        }
      }
      if (done) {  // the sample's value is rad; the lane's next sample starts in the next iteration
        sum = sum + rad;
        ++s;
        fresh = true;
      }
    }
  }
  if (!active) return;
  const size_t p = (size_t)py * (size_t)C.width + (size_t)px;
  accum[p * 3 + 0] = sum.x;
  accum[p * 3 + 1] = sum.y;
  accum[p * 3 + 2] = sum.z;
}

template <int THREADS, int MODE, bool MIS>
static hipError_t launch_nee_1(const DScene& S, const DCamera& C, uint64_t seed, int s_begin, int s_end, int max_depth,
                               const DLight* lights, int n_lights, const int32_t* prim_light, double* accum,
                               hipStream_t stream) {
  const int tiles_x = (C.width + kTile - 1) / kTile, tiles_y = (C.height + kTile - 1) / kTile;
  const int n_tiles = tiles_x * tiles_y;
  const int per_block = THREADS / kWave;
  const int blocks = (n_tiles + per_block - 1) / per_block;
  const size_t lds = trace_lds_bytes(S.n_lds_nodes4, node4_bytes(false), MODE == kSceneLds ? S.n_lds_prims : 0,
                                     MODE == kSceneLds ? S.n_lds_perlin : 0, S.stack_depth4, THREADS,
                                     MODE == kSceneLds ? S.n_lds_mats : 0, MODE == kSceneLds ? S.n_lds_texs : 0);
  hipError_t e = hipFuncSetAttribute((const void*)nee_kernel<THREADS, MODE, MIS>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((nee_kernel<THREADS, MODE, MIS>), dim3(blocks), dim3(THREADS), lds, stream, S, C, seed, s_begin,
                     s_end, max_depth, tiles_x, n_tiles, lights, n_lights, prim_light, accum);
  return hipGetLastError();
}

template <bool MIS>
static hipError_t launch_nee_m(const DScene& S, bool wide, const DCamera& C, uint64_t seed, int s_begin, int s_end,
                               int max_depth, const DLight* lights, int n_lights, const int32_t* prim_light,
                               double* accum, hipStream_t stream) {
  if (wide) {
    if (S.n_lds_prims > 0)
      return launch_nee_1<kNeeThreadsWide, kSceneLds, MIS>(S, C, seed, s_begin, s_end, max_depth, lights, n_lights, prim_light, accum, stream);
    return launch_nee_1<kNeeThreadsWide, kNodesLds, MIS>(S, C, seed, s_begin, s_end, max_depth, lights, n_lights, prim_light, accum, stream);
  }
  const int mode = S.n_lds_nodes4 >= S.n_nodes4 ? kNodesLds : (S.n_lds_nodes4 == 0 ? kNodesGlobal : kNodesMixed);
  switch (mode) {
    case kNodesLds: return launch_nee_1<kHitThreads, kNodesLds, MIS>(S, C, seed, s_begin, s_end, max_depth, lights, n_lights, prim_light, accum, stream);
    case kNodesGlobal: return launch_nee_1<kHitThreads, kNodesGlobal, MIS>(S, C, seed, s_begin, s_end, max_depth, lights, n_lights, prim_light, accum, stream);
    default: return launch_nee_1<kHitThreads, kNodesMixed, MIS>(S, C, seed, s_begin, s_end, max_depth, lights, n_lights, prim_light, accum, stream);
  }
}

// rt_render_nee: block and placement chosen as launch_features does
hipError_t launch_nee(const DScene& S, bool wide, bool mis, const DCamera& C, uint64_t seed, int s_begin, int s_end,
                      int max_depth, const DLight* lights, int n_lights, const int32_t* prim_light, double* accum,
                      hipStream_t stream) {
  if (S.exts) return hipErrorInvalidValue;  // (the caller refuses book-2 scenes)
  if (!accum || !prim_light || (n_lights > 0 && !lights)) return hipErrorInvalidValue;
  return mis ? launch_nee_m<true>(S, wide, C, seed, s_begin, s_end, max_depth, lights, n_lights, prim_light, accum, stream)
             : launch_nee_m<false>(S, wide, C, seed, s_begin, s_end, max_depth, lights, n_lights, prim_light, accum, stream);
}

}  // namespace rt
