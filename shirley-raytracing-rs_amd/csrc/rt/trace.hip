// trace.hip — MI355X (gfx950) path-tracing kernels for the reference's ray_color() hot path.
//
// Semantics follow the reference line by line (citations below); arithmetic is binary64 like the
// reference (core/math.rs:5) and the file is compiled with -ffp-contract=off (Rust never fuses).
//
// Execution model (MI355X-first):
//   * persistent waves: every lane owns one work unit = (pixel, chunk of samples) and runs the
//     reference's bounce loop one segment per iteration; a lane whose path ends starts its next
//     sample at once (path regeneration), a lane whose unit ends takes a new unit from the wave's
//     64-unit window (ballot + popcount rank, one global atomic per 64 units);
//   * units are enumerated tile-major (8x8 pixel tile x sample chunk x lane), so a fresh window
//     hands a wave 64 neighbouring pixels: coherent primary rays;
//   * 4-wide collapsed BVH with conservative f32 child boxes (160-B DNode4F) and exact f64 leaf
//     tests, nearest-first traversal, per-lane stack in LDS laid out [depth][lane] (conflict-free
//     at any depth); for scenes that fit, the nodes, primitives and Perlin tables live in LDS too
//     (one 1024-thread block per CU: 4 waves per SIMD at 128 VGPRs);
//   * Perlin marble octaves and rejection-sampling attempts of a segment are dealt across the whole
//     wave (marble_coop, random_in_unit_sphere_coop);
//   * per-unit partial sums go to HBM once; a reduce kernel sums chunks in order (deterministic).
#include "adaptive.h"
#include "rt_device.h"
#include "pass_frame.h"
#include "rt_launch.h"

#include <algorithm>
#include <vector>

namespace rt {

// ------------------------------------------------------------------------------------------
// persistent trace kernel
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long lanemask_lt() {
  unsigned lane = __lane_id();
  return (lane == 0) ? 0ull : ((~0ull) >> (64 - lane));
}

// LDS of a block: [n_lds_nodes x DNode][stack_depth x STRIDE int][stack_depth x STRIDE float]
__host__ __device__ inline size_t lds_bytes(int n_lds_nodes, int stack_depth, int stride) {
  return (size_t)n_lds_nodes * sizeof(DNode) + (size_t)stack_depth * stride * 8;
}

// THREADS = kTraceThreads (256-thread blocks, several per CU, at least 4 waves per SIMD: 128 VGPRs)
// or kTraceThreadsWide (one 1024-thread block per CU whose LDS holds the scene next to the stacks:
// 4 waves per SIMD, 128 VGPRs).  HIP's second launch-bounds argument is the minimum waves per SIMD.
// EXT: the scene has book-2 primitives; their code is compiled into separate
// instances so that reference scenes keep the kernel's register allocation.
#ifndef RT_KSCENE
#define RT_KSCENE 1
#endif
// Minimum waves per SIMD of the 256-thread instances (4 = 128 VGPRs: 3 and 5 measured slower);
// the book-2 ones at 3 (168 VGPRs: ~90 spilled VGPRs at 4; final_scene on them +27 %).
#ifndef RT_NARROW_WAVES
#define RT_NARROW_WAVES 4
#endif
constexpr int kNarrowWaves = RT_NARROW_WAVES;
#ifndef RT_NARROW_WAVES_EXT
#define RT_NARROW_WAVES_EXT 3
#endif

// LIST: the launch's tiles come from DWork.tile_list (an adaptive step, adaptive.h) — separate instances, so
// that every other call runs the code it ran without the list.
// HOP: the hop pass at the end of the iteration body (below) — 0: none; 1: by a visit of the tree's first node;
// 2: from the scene's ground stack (ScenePlacement.hop_kind); 3: the same with the down pass after the traversal
// (ScenePlacement.hop_down); 4: 3 on a plane stack, both passes by the closed-form next plane
// (ScenePlacement.hop_planes) — compiled only into the scene-in-LDS
// reference-scene instances that launch_trace picks for a scene with a dielectric RectBox (ScenePlacement.hop_pass),
// so every other instance keeps its code.
#ifndef RT_HOP_MIN_LANES
// the pass runs when at least this many lanes of the wave are candidates: 40 of {1, 8, 12, 16, 24, 32, 40, 48}
// (the pass is ~3100 instructions of divergent leaf loops, so it pays only on waves looking at
// the ground)
#define RT_HOP_MIN_LANES 40
#endif
// HOP = 2 (a scene with a ground stack): the lane thresholds of the pass's first run and of its second run,
// whose candidates are the lanes the first run served: 24 / 16 of a sweep from 16 / 8 to 40 / 32.
// RT_HOP2_INSIDE = 0 (A/B only) counts every rect / RectBox continuation as a candidate, like HOP = 1: best
// +2.1 % at 32 / 24 against +4.7 % with the inward-ray filter.
#ifndef RT_HOP2_INSIDE
#define RT_HOP2_INSIDE 1
#endif
#ifndef RT_HOP2_MIN_LANES_A
#define RT_HOP2_MIN_LANES_A 24
#endif
#ifndef RT_HOP2_MIN_LANES_B
#define RT_HOP2_MIN_LANES_B 16
#endif
// HOP = 3 (a ground stack with a non-dielectric member below its coat, ScenePlacement.hop_down): HOP = 2's pass plus
// the down pass between the traversal and the hit record (below).  The lane thresholds of its up to three runs —
// 32 / 16 / 16 of a sweep from 8 / 8 / 8 to 48 / 16 / 16 — and those of step 5's two runs in this instance, whose
// candidates the down pass changes: 24 / 16 of {20 / 16, 24 / 8, 24 / 16, 24 / 24, 32 / 16} re-swept at 32 / 16 / 16
// (20 / 16 is +0.3 %, inside the sweep's spread).
#ifndef RT_HOPD_MIN_LANES_A
#define RT_HOPD_MIN_LANES_A 32
#endif
#ifndef RT_HOPD_MIN_LANES_B
#define RT_HOPD_MIN_LANES_B 16
#endif
#ifndef RT_HOPD_MIN_LANES_C
#define RT_HOPD_MIN_LANES_C 16
#endif
#ifndef RT_HOP3_MIN_LANES_A
#define RT_HOP3_MIN_LANES_A RT_HOP2_MIN_LANES_A
#endif
#ifndef RT_HOP3_MIN_LANES_B
#define RT_HOP3_MIN_LANES_B RT_HOP2_MIN_LANES_B
#endif
// HOP = 4 (HOP = 3 on a plane stack, ScenePlacement.hop_planes): the same two passes with plane_hop_t for the stack's
// answer — no general ground_hop_t code in the instance.  Its own thresholds, re-swept with the cheaper run: the down
// pass at 24 / 16 / 16 and step 5' at 16 / 8 (profiles/planehop/threshold_sweep.jsonl), and the down
// pass's first run at 20 with serve_y's cheaper serve body (RT_SERVE_Y below; profiles/servey/threshold_sweep.jsonl).
#ifndef RT_HOP4D_MIN_LANES_A
#define RT_HOP4D_MIN_LANES_A (RT_SERVE_Y ? 20 : 24)
#endif
#ifndef RT_HOP4D_MIN_LANES_B
#define RT_HOP4D_MIN_LANES_B RT_HOPD_MIN_LANES_B
#endif
#ifndef RT_HOP4D_MIN_LANES_C
#define RT_HOP4D_MIN_LANES_C RT_HOPD_MIN_LANES_C
#endif
#ifndef RT_HOP4_MIN_LANES_A
#define RT_HOP4_MIN_LANES_A 16
#endif
#ifndef RT_HOP4_MIN_LANES_B
#define RT_HOP4_MIN_LANES_B 8
#endif
// ... and, in the same two instances, the traversal itself settles the stack's primitives by closed form before its
// first visit (rt_device.h plane_first, traverse4 GF).  0 builds the A/B partner (tools/variant.sh).
#ifndef RT_GROUND_FIRST
#define RT_GROUND_FIRST 1
#endif
// ... and both passes shade a hit on a y face of a RectBox by the serve body written out for its axis normal
// (rt_device.h serve_y).  0 builds the A/B partner with the general body alone (tools/variant.sh).
#ifndef RT_SERVE_Y
#define RT_SERVE_Y 1
#endif
#ifdef RT_HOP_SERVE_SHARED
// A/B only: the serve body of the HOP = 3 instances as one call that the down pass and step 5' both
// reach, instead of an inlined copy at each site.  Not built by default: the two inlined sites measured faster.
struct ServeOut {
  v3 o, d;
  uint32_t draw, c2, c3;
};
__device__ __noinline__ ServeOut hop_serve_ool(const DPrim* lds_prims, const DMat* mats, int prim, int face, v3 o, v3 d,
                                               double t, Rng rng, uint64_t seed_v) {
  DScene S{};  // (hit_record reads the scene only for book-2 primitives)
  const uint64_t seed = uniform64(seed_v);
  const DPrim pr = lds_prims[prim];
  Hit hh;
  hit_record<false, false>(S, pr, face, o, d, t, rng, seed, hh);
  const v3 ru = draw_diel(rng, seed);
  const v3 ud = unit_fast(d);
  shade_dielectric(mats[pr.material], ru, ud, rng, o, d, hh);
  return ServeOut{o, d, rng.draw, rng.c2, rng.c3};
}
#endif
template <int THREADS, int MODE, bool EXT, bool LIST = false, int HOP = 0>
__global__ __launch_bounds__(THREADS, THREADS >= kTraceThreadsWide3 ? 1 : (EXT ? RT_NARROW_WAVES_EXT : kNarrowWaves))
void trace_kernel(KParams P) {
  extern __shared__ unsigned char lds_raw[];
  const int tid = threadIdx.x;
  typedef typename Node4Sel<EXT>::T N4;
  N4* lds_nodes = reinterpret_cast<N4*>(lds_raw);
  DPrim* lds_prims = reinterpret_cast<DPrim*>(lds_raw + (size_t)P.scene.n_lds_nodes4 * sizeof(N4));
  const DPerlin* lds_perlin = (MODE == kSceneLds && P.scene.n_lds_perlin > 0)
                                  ? reinterpret_cast<const DPerlin*>(lds_prims + P.scene.n_lds_prims)
                                  : nullptr;
  unsigned char* stk_base = lds_raw + (size_t)P.scene.n_lds_nodes4 * sizeof(N4) +
                            (MODE == kSceneLds ? (size_t)P.scene.n_lds_prims * sizeof(DPrim) +
                                                     (size_t)P.scene.n_lds_perlin * sizeof(DPerlin) +
                                                     (size_t)P.scene.n_lds_mats * sizeof(DMat) +
                                                     (size_t)P.scene.n_lds_texs * sizeof(DTex)
                                               : 0);
  unsigned* stk = reinterpret_cast<unsigned*>(stk_base) + tid;  // [stack_depth4][THREADS] packed entries
  stage_nodes4<MODE>(P.scene, lds_nodes, lds_prims);
  // the material and texture tables: the scene-in-LDS block's copies (after the Perlin tables: the host
  // places the primitives in LDS only together with them), else global memory.  Unconditional per
  // instance, so the compiler reads the LDS copies with ds_read (a runtime choice made every read a FLAT
  // load).
  const DMat* mats = P.scene.mats;
  const DTex* texs = P.scene.texs;
  if constexpr (MODE == kSceneLds) {
    mats = reinterpret_cast<const DMat*>(reinterpret_cast<const DPerlin*>(lds_prims + P.scene.n_lds_prims) +
                                         P.scene.n_lds_perlin);
    texs = reinterpret_cast<const DTex*>(mats + P.scene.n_lds_mats);
  }

  const DCamera& C = P.cam;
  const DWork& W = P.work;
  const uint64_t seed = W.seed;
  const int lane = __lane_id();

  // wave-uniform window of unit indices
  unsigned long long w_next = 0, w_end = 0;
  bool exhausted = false;
  // units are taken from per-block segments of the unit space (stealing from other segments once the
  // block's is empty) when DWork.n_segs != 0, else from one global queue.
  // the block's segment, XCD-major: blocks are dealt round-robin to the 8 XCDs, so block b (on XCD
  // b % 8) owns segment (b % 8) * ceil(n / 8) + b / 8 — an XCD's blocks own adjacent segments
  uint32_t seg;
  {
    const uint32_t per_xcd = (W.n_segs + 7u) / 8u, s0 = (blockIdx.x % 8u) * per_xcd + blockIdx.x / 8u;
    seg = s0 < W.n_segs ? s0 : blockIdx.x % max(W.n_segs, 1u);
  }

  // lane state
  // (kept lean: every loop-carried VGPR here competes with the 128-VGPR budget of 4 waves per SIMD)
  bool has_unit = false, active = false;
  uint32_t pxy = 0;   // px | py << 16 of the unit's pixel (the host keeps width, height <= 65535)
  int s_end = 0;      // the unit's samples are [.., s_end); the current one is rng.sample
  uint32_t part_index = 0;  // partial-buffer slot of the unit (the host keeps slots < 2^32)
  v3 sum = V(0, 0, 0), o = V(0, 0, 0), d = V(0, 0, 0), att = V(0, 0, 0), em = V(0, 0, 0);
  int depth_left = 0;
  Rng rng{0, 0, 0, 0, 0};
  unsigned long long n_seg = 0, n_samp = 0;  // wave-uniform (SGPRs): popcounts of ballots
  unsigned visits = 0, ptests = 0;           // per lane; flushed to the counters before 2^31

#ifdef RT_PHASE_TIMING
  // wave-uniform clock stamps at wave-uniform points of the loop (SGPR sums): the iteration's time by
  // phase (kPh* buckets), plus the traversal step statistics
  unsigned long long ph_t[kPhBuckets] = {}, ph_last = clock64(), ph_lane_steps = 0, ph_wave_steps = 0;
#define PH_STAMP(b)                               \
  do {                                            \
    const unsigned long long ph_now = clock64();  \
    ph_t[b] += ph_now - ph_last;                  \
    ph_last = ph_now;                             \
  } while (0)
  // ... and, inside a run of the hop passes, the wave's cycles by part (serve body / next hit with its guard read):
  // begun and added by the same set of lanes, one of which adds the wave's cycles to g_hop_clk
  unsigned long long ph_part_last = 0;
#define PH_PART_BEGIN() ph_part_last = clock64()
#define PH_PART(b)                                                                                                \
  do {                                                                                                            \
    const unsigned long long ph_now = clock64();                                                                  \
    if ((int)__lane_id() == __builtin_ctzll(__ballot(1))) atomicAdd(&g_hop_clk[b], ph_now - ph_part_last);        \
    ph_part_last = ph_now;                                                                                        \
  } while (0)
#else
#define PH_STAMP(b) \
  do {              \
  } while (0)
#define PH_PART_BEGIN() \
  do {                  \
  } while (0)
#define PH_PART(b) \
  do {             \
  } while (0)
#endif
#ifdef RT_TIMELINE
  const unsigned wave_gid = blockIdx.x * (THREADS / kWave) + tid / kWave;
  bool ph_exh_seen = false;
  if (lane == 0 && wave_gid < (unsigned)kTimelineWaves) g_wave_t0[wave_gid] = __builtin_amdgcn_s_memrealtime();
#endif
  // One iteration: (1) a ray_color segment for every lane holding a path (closest hit, record,
  // material); (2) lanes whose path ends here (sky or a light) or that hold none take the next sample
  // of their unit or a new unit; (3) one wave-wide sampler draws everything the iteration needs — the
  // scatters' unit-sphere points, the dielectrics' uniforms and the new samples' jitter + lens points;
  // (4) shading; ended lanes add their radiance and publish finished units; new samples' camera rays.
  for (;;) {
#if defined(RT_PHASE_TIMING) && !defined(RT_PHASE_NO_EVENTS)
    const unsigned long long ph_before = ph_lane_steps;
#endif
    // the scene record: the kernel argument's copy for every instance.  (Round 5 had the book-2 instances
    // re-read it from the pass's KBlock with scalar loads each iteration, +0.2 % then; with the extended
    // objects' tests moved out of the traversal loop the argument copy is +1.1 % on final_scene:
    // 1675 / 1676 vs 1657 / 1655 Msamples/s, gpurun_out/r06n)
    const DScene& S = P.scene;
    // 1. one ray_color iteration (render.rs:30-46): closest hit and hit record, the material and the
    // texture leaf of a diffuse / emitting material
    bool hit = false, need_pn = false, need_r = false;
    int prim = -1, face = -1, leaf = -1, mat = 0, ptab = 0, mk = -1;
    double t_best = __builtin_inf(), psc = 0.0;
    Hit h;
    h.point = V(0.0, 0.0, 0.0);
    h.normal = h.point;
    h.t = h.u = h.v = 0.0;
    h.front_face = false;
    PH_COUNT(6);
    n_seg += __popcll(__ballot(active));
    // 1'. the down pass (HOP = 3, 4).  A lane whose traversal hit is a dielectric primitive of the
    // ground stack — the coat's top from above, mostly — is shaded here by the hop pass's serve body and asks the
    // stack for its next hit (ground_hop_t<true>; HOP = 4: plane_hop_t<true>): a dielectric one, served, sends it round again (up to three
    // runs, each with its own lane threshold); any other one that the stack's conditions prove the scene's closest —
    // the rect under the coat — becomes the lane's hit of this iteration, recorded, sampled and shaded by the
    // ordinary steps below; step 5 then takes the lane up through the coat.  One ground interaction is one
    // iteration.  A lane that the stack cannot answer (or whose ray left the box it hit) waits: it keeps its new ray,
    // takes no part in the steps below and traverses from the root next iteration, as it would have anyway.  The
    // same functions of (seed, pixel, sample, draw index, ray) in each lane's own order as the iterations it
    // replaces: frames and counters are bit-identical with and without the pass.
    bool waiting = false;
    if constexpr (HOP >= 3) {
      static_assert(MODE == kSceneLds && !EXT, "the hop pass is built for the scene-in-LDS reference-scene instances");
      // (the pass's ballots need a wave-uniform point: this instance traverses here, not in the block below)
      // (the stack's record: read before the traversal where the traversal itself asks it, else after, as before)
      constexpr bool kFirst = HOP == 4 && RT_GROUND_FIRST;
      GGround* g;
      if constexpr (kFirst) g = (GGround*)kblock(P.kconst)->ground;
      if (active) {
        if constexpr (kFirst)
          prim = traverse4<THREADS, MODE, EXT, true>(S, lds_nodes, lds_prims, o, d, 0.001, t_best, face, stk, rng, seed,
                                                     visits, ptests RT_STAT_ARG(ph_lane_steps), g,
                                                     (GPlanes*)kblock(P.kconst)->planes);
        else
          prim = traverse4<THREADS, MODE, EXT>(S, lds_nodes, lds_prims, o, d, 0.001, t_best, face, stk, rng, seed, visits,
                                               ptests RT_STAT_ARG(ph_lane_steps));
      }
      PH_STAMP(kPhTrav);
      if constexpr (!kFirst) g = (GGround*)kblock(P.kconst)->ground;
      bool pend = false;  // a dielectric hit of G in (prim, face, t_best), not shaded yet
      if (active && prim >= 0 && mats[lds_prims[prim].material].kind == RT_MAT_DIELECTRIC)
        for (int i = 0; i < g->n; ++i) pend = pend || g->prim[i] == prim;
#if defined(RT_PHASE_TIMING) && !defined(RT_PHASE_NO_EVENTS)
      if (pend) PH_COUNT(31);
#endif
#pragma unroll 1
      for (int run = 0; run < 3; ++run) {
        if (__popcll(__ballot(pend)) <
            (HOP == 4 ? (run == 0 ? RT_HOP4D_MIN_LANES_A : (run == 1 ? RT_HOP4D_MIN_LANES_B : RT_HOP4D_MIN_LANES_C))
                      : (run == 0 ? RT_HOPD_MIN_LANES_A : (run == 1 ? RT_HOPD_MIN_LANES_B : RT_HOPD_MIN_LANES_C))))
          break;
        int kind = kHopRefused;
        if (pend) {
          PH_COUNT(36 + 4 * run);
          PH_PART_BEGIN();
          pend = false;
#ifdef RT_HOP_SERVE_SHARED
          const ServeOut so = hop_serve_ool(lds_prims, mats, prim, face, o, d, t_best, rng, seed);
          o = so.o, d = so.d, rng.draw = so.draw, rng.c2 = so.c2, rng.c3 = so.c3;
#else
          if constexpr (HOP == 4 && RT_SERVE_Y) {
            // (a y face — nearly every hit the traversal hands the pass — by serve_y; a side face, or a lane serve_y
            // sends back, by the general body)
            const DMat& dm = mats[lds_prims[prim].material];
            const v3 ru = draw_diel(rng, seed);
            const bool by_y = face >= 4 && serve_y(dm, ru, rng, o, d, t_best);
            if (by_y) PH_COUNT(51);
            if (!by_y) {
              PH_COUNT(52);
              const DPrim pr = lds_prims[prim];
              Hit hh;
              hit_record<false, false>(S, pr, face, o, d, t_best, rng, seed, hh);
              shade_dielectric(dm, ru, unit_fast(d), rng, o, d, hh);
            }
          } else {
          const DPrim pr = lds_prims[prim];
          Hit hh;
          hit_record<false, false>(S, pr, face, o, d, t_best, rng, seed, hh);
          const v3 ru = draw_diel(rng, seed);
          const v3 ud = unit_fast(d);
          shade_dielectric(mats[pr.material], ru, ud, rng, o, d, hh);  // (att * 1 = att, no emission)
          }
#endif
          if (--depth_left <= 0) {
            sum = sum + em;
            active = false;  // takes its next sample in this iteration's step 2
          }
          // (who tries: a ray that runs on inside the box it hit, as in step 5', or downwards out of it, towards
          // what lies under it in the stack; one that left upwards meets the spheres or the sky, and waits)
          const bool inward = face < 0 || d.y < 0.0 || box_inward(face, d);
          PH_PART(kHopClkDownServe);
          prim = -1;
          waiting = active;
          if (active && inward) {
            PH_COUNT(48 + run);  // (asks the stack: served + found answered, the rest declined or refused)
            double t_hop;
            int p_hop, f_hop;
            bool guarded;
            if constexpr (HOP == 4)
              kind = plane_hop_t<true>(g, (GPlanes*)kblock(P.kconst)->planes, o, d, 0.001, t_hop, p_hop, f_hop, guarded);
            else
              kind = ground_hop_t<true>(S, lds_prims, mats, g, o, d, 0.001, t_hop, p_hop, f_hop, guarded);
            if (kind != kHopRefused) {
              prim = p_hop;
              face = f_hop;
              t_best = t_hop;
              waiting = false;
              pend = kind == kHopServed;
              if (pend) PH_COUNT(37 + 4 * run); else PH_COUNT(38 + 4 * run);
            }
          }
          PH_PART(kHopClkDownNext);
          if (waiting) PH_COUNT(39 + 4 * run);
        }
        n_seg += __popcll(__ballot(kind != kHopRefused));
      }
      PH_STAMP(kPhDown);
    }
    if (active) {
      if constexpr (HOP < 3)
        prim = traverse4<THREADS, MODE, EXT>(S, lds_nodes, lds_prims, o, d, 0.001, t_best, face, stk, rng, seed, visits,
                                        ptests RT_STAT_ARG(ph_lane_steps));
#ifdef RT_PHASE_TIMING
    }  // (instrumented build: the traversal's stamp at a wave-uniform point)
    PH_STAMP(kPhTrav);
    {
#endif
      if (prim >= 0) {
        PH_COUNT(15);
        hit = true;
        const DPrim pr = (MODE == kSceneLds) ? lds_prims[prim] : S.prims[prim];  // (LDS copy when resident)
        hit_record<false, EXT>(S, pr, face, o, d, t_best, rng, seed, h);
        mat = pr.material;
        mk = mats[mat].kind;
        need_r = mk == RT_MAT_LAMBERTIAN || mk == RT_MAT_METAL || mk == RT_MAT_FAIRY_LIGHT || mk == RT_MAT_ISOTROPIC;
        if (mk == RT_MAT_LAMBERTIAN || mk == RT_MAT_FAIRY_LIGHT || mk == RT_MAT_DIFFUSE_LIGHT || mk == RT_MAT_ISOTROPIC) {
          leaf = resolve_texture_t(texs, mats[mat].tex, h.point);
          const DTex& tx = texs[leaf];
          if (tx.kind == RT_TEX_PERLIN) {
            need_pn = true;
            ptab = tx.table;
            psc = tx.scale;
          }
        }
      }
    }
    PH_STAMP(kPhRecord);
#if defined(RT_PHASE_TIMING) && !defined(RT_PHASE_NO_EVENTS)
    // (instrumented build: how the lanes that a pass between the traversal and the sampler could take — those whose
    // traversal hit is a dielectric primitive of the ground stack — are bunched in the wave)
    if constexpr (HOP == 2) {
      bool dg = false;
      if (hit && mk == RT_MAT_DIELECTRIC) {
        GGround* g = (GGround*)kblock(P.kconst)->ground;
        for (int i = 0; i < g->n; ++i) dg = dg || g->prim[i] == prim;
      }
      const int n_dg = __popcll(__ballot(dg));
      if (dg) {
        PH_COUNT(31);
        if (n_dg >= 8) PH_COUNT(32);
        if (n_dg >= 16) PH_COUNT(33);
        if (n_dg >= 24) PH_COUNT(34);
        if (n_dg >= 32) PH_COUNT(35);
      }
    }
#endif
    // 2. the path ends at this segment when it misses (the sky) or meets a material that does not
    // scatter (diffuse light): known before shading, so the lane's next sample starts in this iteration
    // (a lane left waiting by the down pass is neither: it holds a path and does nothing until the next iteration)
    const bool ends = active && !waiting && (!hit || mk == RT_MAT_DIFFUSE_LIGHT);
    const bool free_lane = !active || ends;
    // a unit whose last sample ends here is published after shading (its sum is complete then)
    bool publish = false;
    uint32_t pub_index = 0;
    if (free_lane && has_unit && rng.sample + 1u >= (uint32_t)s_end) {
      publish = true;
      pub_index = part_index;
      has_unit = false;
    }
    // lanes without a unit take one from the wave's window (one global atomic per 64 units)
    bool need = free_lane && !has_unit;
    unsigned long long mask = __ballot(need);
    if (mask != 0ull && !exhausted) {
      unsigned long long k = __popcll(mask);
      unsigned long long rank = __popcll(mask & lanemask_lt());
      unsigned long long avail = w_end - w_next;
      unsigned long long idx;
      unsigned win = kSegmentWindow;  // units of the window taken below
      if (avail >= k) {
        idx = w_next + rank;
        w_next += k;
      } else {
        KBlk* kb = kblock(P.kconst);  // (the queue's pointers and sizes, read with scalar loads here)
        unsigned long long nb = kb->work.n_units;
        if (kb->work.n_segs != 0u) {
        // the block's segment (consecutive chunks of neighbouring tiles: coherent lanes, the same
        // subtrees in this XCD's L2), then any segment that still holds units: the 64 lanes read 64
        // candidates' counters at once (device-coherent atomic loads) and the wave takes the first
        // non-empty one.  A failed take means that segment is now empty for good (counters only grow),
        // so the search ends after at most n_segs failures.
        unsigned* ctr = reinterpret_cast<unsigned*>(kb->unit_counter);
        for (;;) {
          unsigned off = 0;
          if (lane == 0) off = atomicAdd(ctr + seg, kSegmentWindow);
          off = (unsigned)__builtin_amdgcn_readfirstlane((int)off);
          const uint32_t seg_len = kb->work.seg_len;
          const unsigned long long n_units = kb->work.n_units;
          if (off < seg_len && (unsigned long long)seg * seg_len + off < n_units) {
            nb = (unsigned long long)seg * seg_len + off;
            break;
          }
          bool found = false;
          const uint32_t n_segs = kb->work.n_segs;
          for (uint32_t base = 0; base < n_segs; base += kWave) {
            uint32_t cand = seg + 1u + base + (uint32_t)lane;
            if (cand >= n_segs) cand -= n_segs;
            bool has = false;
            if (base + (uint32_t)lane < n_segs) {
              const unsigned o = __hip_atomic_load(ctr + cand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              has = o < seg_len && (unsigned long long)cand * seg_len + o < n_units;
            }
            const unsigned long long m = __ballot(has);
            if (m != 0ull) {
              seg = (uint32_t)__builtin_amdgcn_readlane((int)cand, (int)__builtin_ctzll(m));
              found = true;
              break;
            }
          }
          if (!found) break;
        }
        } else {  // one shared queue (short units: DWork.n_segs = 0), q_window units per atomic (plan.h)
          win = kb->work.q_window;
          nb = 0;
          if (lane == 0) nb = atomicAdd(kb->unit_counter, (unsigned long long)win);
          nb = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(nb >> 32)) << 32) |
               (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)nb);
        }
        idx = (rank < avail) ? (w_next + rank) : (nb + (rank - avail));
        w_next = nb + (k - avail);
        w_end = nb + win;
        if (nb >= W.n_units) exhausted = true;
      }
      if (need && idx < W.n_units) {
        KBlk* kb = kblock(P.kconst);
        // unit -> (local tile, chunk, lane-in-tile); tile-major so a window = 64 neighbours.  32-bit
        // quotients (the host keeps n_units < 2^32): far cheaper than 64-bit ones.  The work
        // descriptor and the image size are read here with scalar loads, like the camera below.
        KWork* kw = &kb->work;
        KCamera* kc = &kb->cam;
        const uint32_t pt = (uint32_t)kw->n_chunks * (uint32_t)kTilePixels, i32 = (uint32_t)idx;
        const uint32_t lt = udiv(i32, UDiv{kw->div_unit_tile.m, kw->div_unit_tile.s1, kw->div_unit_tile.s2});  // i32 / pt
        uint32_t g32;
        if constexpr (LIST) {
          // an adaptive step's launch names its tiles in a list (DWork.tile_list, read here like the rest
          // of the descriptor: not held across the loop)
          typedef __attribute__((address_space(1))) const uint32_t GTile;
          g32 = ((GTile*)kw->tile_list)[lt];
        } else {
          g32 = lt * (uint32_t)kw->tile_world + (uint32_t)kw->tile_rank;
        }
        const uint32_t y32 = udiv(g32, UDiv{kw->div_tiles_x.m, kw->div_tiles_x.s1, kw->div_tiles_x.s2});  // g32 / tiles_x
        const uint32_t rem = i32 - lt * pt;
        const int tx = (int)(g32 - y32 * (uint32_t)kw->tiles_x);
        const int ty = kw->ty0 + (int)y32;
        int chunk = (int)(rem / kTilePixels);
        int lp = (int)(rem % kTilePixels);
        const int px = tx * kTile + (lp % kTile);
        const int py = ty * kTile + (lp / kTile);
        if (px < kc->width && py < kc->height) {
          PH_COUNT(10);
          has_unit = true;
          const int s0 = kw->sample_base + chunk * kw->chunk;
          s_end = min(kw->samples, s0 + kw->chunk);
          rng.sample = (uint32_t)s0 - 1u;  // advanced before each sample (wraps to s0)
          rng.pixel = (uint32_t)py * (uint32_t)kc->width + (uint32_t)px;
          pxy = (uint32_t)px | ((uint32_t)py << 16);
          part_index = (uint32_t)chunk * ((uint32_t)kw->n_tiles_rank * (uint32_t)kTilePixels) +
                       lt * (uint32_t)kTilePixels + (uint32_t)lp;
        }
      }
    }
    // a free lane holding a unit starts its next sample (render.rs:60-65): draws from 0 again
    const bool regen = free_lane && has_unit;
    n_samp += __popcll(__ballot(regen));
    if (regen) {
      rng.sample += 1u;
      rng.draw = 0;
    }
    PH_STAMP(kPhRegen);
    // 3. Perlin marble values for the lanes that need one, by the whole wave (wave-uniform)
    const double pn = lds_perlin ? marble_coop((LdsPerlin*)lds_perlin, need_pn, ptab, psc, h.point)
                                 : marble_coop(S.perlin, need_pn, ptab, psc, h.point);
    PH_STAMP(kPhMarble);
    // every draw of the iteration, by the wave: the scatter's random_in_unit_sphere, the dielectric's
    // uniform, a new sample's jitter and lens point
    const bool scat = active && !ends && !waiting;
    const int dk = regen ? kDrawCam
                         : (scat && need_r) ? kDrawSphere : (scat && mk == RT_MAT_DIELECTRIC) ? kDrawDiel : kDrawNone;
    double jx = 0.0, jy = 0.0;
    const v3 rs = draws_coop(rng, seed, dk, C.has_lens != 0, pxy, jx, jy);
    // the one normalisation a lane's shading needs, for all lanes at once: unit(r) for a lambertian /
    // fairy light scatter, unit(d) for dielectric, metal and the sky (others: a dummy)
    const v3 un = unit_fast(!active ? V(1.0, 1.0, 1.0) : (scat && need_r && mk != RT_MAT_METAL) ? rs : d);
    PH_STAMP(kPhDraws);
    // 4. emitted + scatter (render.rs:31-45) or the sky; an ended lane's o, d are free once un holds
    // unit(d), so its new sample's camera ray is formed first
    if (regen) {
      PH_COUNT(11);
      // the camera read with scalar loads here (an opaque copy of its address keeps them from being
      // hoisted): held in SGPRs across the loop it spills to VGPR lanes, ~66 v_readlane per iteration
      camera_ray_drawn(kblock(P.kconst)->cam, jx, jy, rs, o, d);
    }
    PH_STAMP(kPhCamera);
    if (active && !waiting) {
      bool alive, has_emit = false;
      v3 mul = V(1.0, 1.0, 1.0), emit = V(0.0, 0.0, 0.0);
      if (hit) {
        const DMat& m = mats[mat];  // (fields read where used: a copy loaded them all up front and spilled them)
        alive = shade_factor(S, texs, m, leaf, pn, rs, un, rng, o, d, h, prim, face, mul, emit, has_emit);
      } else {
        PH_COUNT(20);
#if RT_KSCENE
        // the sky's kind and colour read with scalar loads here, like the camera (held in SGPRs across
        // the loop they spill to VGPR lanes)
        emit = sky_unit(kblock(P.kconst)->scene, un);
#else
        emit = sky_unit(S, un);
#endif
        has_emit = true;
        alive = false;
      }
      // the path's throughput and radiance, read and written once per segment
      if (has_emit) em = em + hmul(att, emit);
      att = hmul(att, mul);
      if (alive) alive = --depth_left > 0;
      if (!alive) {
        sum = sum + em;  // c += ray_color(...)
        active = false;
      }
    }
    PH_STAMP(kPhShade);
    // a finished unit publishes its in-order sample sum (render.rs:58-69: *buf_c = c)
    if (publish) {
      PH_COUNT(24);
      double* dst = kblock(P.kconst)->partial + (size_t)pub_index * 3;
      dst[0] = sum.x;
      dst[1] = sum.y;
      dst[2] = sum.z;
      sum = V(0.0, 0.0, 0.0);
    }
    if (regen) {
      att = V(1.0, 1.0, 1.0);
      em = V(0.0, 0.0, 0.0);
      depth_left = kblock(P.kconst)->work.max_depth;  // >= 1: max_depth == 0 frames are written by render_window itself
      active = true;
    }
    PH_STAMP(kPhTail);
    // 5. the hop pass.  The reference scene's ground is a 0.01-thick dielectric RectBox coat over a Lambertian
    // rect: each ground interaction adds segments whose closest hit is found at the tree's first node (the
    // coat's far face from inside it, the coat from the rect), yet each holds its lane for a whole iteration
    // whose length the other lanes' 5-9 node visits set.  A lane that goes on from a rect or RectBox hit tries
    // its next segment here: when the first node decides the closest hit (traverse4_root) and that hit is a
    // dielectric, the segment is done now — the same functions of (seed, pixel, sample, draw index, ray) in
    // the same per-lane order as an iteration's steps 1, 3 and 4, so frames and counters are bit-identical
    // with and without the pass.  Any other lane keeps its ray untouched and traverses from the root in the
    // next iteration as before.  Wave-uniform: run only with enough candidates to pay for the wave's trip.
    if constexpr (HOP == 1) {
      static_assert(MODE == kSceneLds && !EXT, "the hop pass is built for the scene-in-LDS reference-scene instances");
      // (candidates by the hit's kind; measured and rejected, DESIGN.md §5: lanes that go on from a dielectric
      // hit, −8 %, and RectBox hits from outside only, no better at any threshold)
      bool cand = active && !regen && hit;
      if (cand) cand = lds_prims[prim].kind != kPrimSphere;
      if (__popcll(__ballot(cand)) >= RT_HOP_MIN_LANES) {
        bool serve = false;
        double t_hop = __builtin_inf();
        int p_hop = -1, f_hop = -1;
        if (cand) {
          PH_COUNT(26);
#ifdef RT_HOP_ROOT_OUTLINE
          const RootHit rh = traverse4_root_ool<MODE>(lds_nodes, lds_prims, S.prims, S.root4, S.key_mask, S.origin_limit,
                                                      o, d, rng, seed);
          serve = rh.ok != 0;
          t_hop = rh.t;
          p_hop = rh.best;
          f_hop = rh.face;
#else
          serve = traverse4_root<MODE>(S, lds_nodes, lds_prims, o, d, 0.001, t_hop, p_hop, f_hop, rng, seed, visits, ptests);
#endif
          if (serve) serve = mats[lds_prims[p_hop].material].kind == RT_MAT_DIELECTRIC;
        }
        n_seg += __popcll(__ballot(serve));
        if (serve) {
          PH_COUNT(27);
          const DPrim pr = lds_prims[p_hop];
          Hit hh;
          hit_record<false, false>(S, pr, f_hop, o, d, t_hop, rng, seed, hh);
          const v3 ru = draw_diel(rng, seed);
          const v3 ud = unit_fast(d);
          shade_dielectric(mats[pr.material], ru, ud, rng, o, d, hh);  // (att * 1 = att, no emission)
          if (--depth_left <= 0) {
            sum = sum + em;
            active = false;  // takes its next sample in the next iteration's step 2
          }
        }
      }
      PH_STAMP(kPhHop);
    }
    // 5'. the hop pass of a scene with a ground stack (HOP = 2, 3; rt_device.h ground_hop; HOP = 4: plane_hop_t<false>,
    // which declines where ground_hop would refuse, and where it cannot tell): the same
    // candidates, but the closest hit comes from the stack's own primitives — at most four, no node visit — and
    // is served where the stack's conditions prove it the scene's closest hit.  That also decides the upward
    // hop inside the coat, which no first-node visit can (the spheres' boxes start on the coat's top plane), so
    // the pass runs twice: the second run's candidates are the lanes the first one served, which turns "coat
    // bottom from below, coat top from inside" into one iteration.  Each run has its own lane threshold.
    if constexpr (HOP >= 2) {
      static_assert(MODE == kSceneLds && !EXT, "the hop pass is built for the scene-in-LDS reference-scene instances");
      bool cand = active && !regen && hit;
      if (cand) cand = lds_prims[prim].kind != kPrimSphere;
#if RT_HOP2_INSIDE
      // (of the lanes that go on from a RectBox face, only those whose new ray runs inside that box — its next
      // hit is the box's far side unless another primitive of the stack intervenes; one that left the box goes
      // on to the rect below or to the sky, which the pass does not serve.  A choice of who tries, not of who is
      // served: DESIGN.md §5)
      if (cand && face >= 0) cand = box_inward(face, d);
#endif
#pragma unroll 1
      for (int run = 0; run < 2; ++run) {
        if (__popcll(__ballot(cand)) < (HOP == 4   ? (run ? RT_HOP4_MIN_LANES_B : RT_HOP4_MIN_LANES_A)
                                        : HOP == 3 ? (run ? RT_HOP3_MIN_LANES_B : RT_HOP3_MIN_LANES_A)
                                                   : (run ? RT_HOP2_MIN_LANES_B : RT_HOP2_MIN_LANES_A)))
          break;
        bool serve = false;
        double t_hop = __builtin_inf();
        int p_hop = -1, f_hop = -1;
        if (cand) {
          if (run) PH_COUNT(28); else PH_COUNT(26);
          PH_PART_BEGIN();
          bool guarded;
          if constexpr (HOP == 4)
            serve = plane_hop_t<false>((GGround*)kblock(P.kconst)->ground, (GPlanes*)kblock(P.kconst)->planes, o, d, 0.001, t_hop,
                                       p_hop, f_hop, guarded) != kHopRefused;
          else
            serve = ground_hop(S, lds_prims, mats, (GGround*)kblock(P.kconst)->ground, o, d, 0.001, t_hop, p_hop, f_hop, guarded);
          PH_PART(kHopClkHopNext);
          if (guarded) PH_COUNT(30);
        }
        n_seg += __popcll(__ballot(serve));
        if (serve) {
          if (run) PH_COUNT(29); else PH_COUNT(27);
          PH_PART_BEGIN();
#ifdef RT_HOP_SERVE_SHARED
          if constexpr (HOP == 3) {
            const ServeOut so = hop_serve_ool(lds_prims, mats, p_hop, f_hop, o, d, t_hop, rng, seed);
            o = so.o, d = so.d, rng.draw = so.draw, rng.c2 = so.c2, rng.c3 = so.c3;
          } else
#endif
          if constexpr (HOP == 4 && RT_SERVE_Y) {  // (as in the down pass: every served hit of a plane stack is a y face)
            const DMat& dm = mats[lds_prims[p_hop].material];
            const v3 ru = draw_diel(rng, seed);
            const bool by_y = f_hop >= 4 && serve_y(dm, ru, rng, o, d, t_hop);
            if (by_y) PH_COUNT(53);
            if (!by_y) {
              PH_COUNT(54);
              const DPrim pr = lds_prims[p_hop];
              Hit hh;
              hit_record<false, false>(S, pr, f_hop, o, d, t_hop, rng, seed, hh);
              shade_dielectric(dm, ru, unit_fast(d), rng, o, d, hh);
            }
          } else {
          const DPrim pr = lds_prims[p_hop];
          Hit hh;
          hit_record<false, false>(S, pr, f_hop, o, d, t_hop, rng, seed, hh);
          const v3 ru = draw_diel(rng, seed);
          const v3 ud = unit_fast(d);
          shade_dielectric(mats[pr.material], ru, ud, rng, o, d, hh);  // (att * 1 = att, no emission)
          }
          if (--depth_left <= 0) {
            sum = sum + em;
            active = false;  // takes its next sample in the next iteration's step 2
          }
          PH_PART(kHopClkHopServe);
        }
        cand = serve && active;
#if RT_HOP2_INSIDE
        if (cand) cand = box_inward(f_hop, d);
#endif
      }
      PH_STAMP(kPhHop);
    }
#ifdef RT_TIMELINE
    if (exhausted && !ph_exh_seen) {
      ph_exh_seen = true;
      if (lane == 0 && wave_gid < (unsigned)kTimelineWaves) g_wave_tx[wave_gid] = __builtin_amdgcn_s_memrealtime();
    }
#endif
    // done when no lane holds a path or a unit and the pool is drained (a lane that fails to get a
    // unit while the pool is not drained — e.g. an edge tile's unit outside the image — retries)
    if (exhausted && !__any(active || has_unit)) break;
#if defined(RT_PHASE_TIMING) && !defined(RT_PHASE_NO_EVENTS)
    {
      unsigned dl = (unsigned)(ph_lane_steps - ph_before);  // this lane's steps (0 when idle)
      if (dl > 0) atomicAdd(&g_visit_hist[min(dl, 63u)], 1ull);
      for (int off = 32; off > 0; off >>= 1) dl = max(dl, (unsigned)__shfl_xor((int)dl, off));
      ph_wave_steps += dl;  // the wave's loop iterations = its slowest lane's steps
      if (lane == 0 && dl > 0) atomicAdd(&g_wave_visit_hist[min(dl, 63u)], 1ull);
    }
#endif
    if (visits > (1u << 30) || ptests > (1u << 30)) {  // (never within a frame of today's sizes)
      DCounters* cs = kblock(P.kconst)->counters + (blockIdx.x % kCounterSlots);
      atomicAdd(&cs->node_visits, (unsigned long long)visits);
      atomicAdd(&cs->prim_tests, (unsigned long long)ptests);
      visits = ptests = 0;
    }
  }
#ifdef RT_TIMELINE
  if (lane == 0 && wave_gid < (unsigned)kTimelineWaves) g_wave_t1[wave_gid] = __builtin_amdgcn_s_memrealtime();
#endif
  // wave-reduce the per-lane counters, one atomic per wave
  unsigned long long n_vis = visits, n_pt = ptests;
  for (int off = 32; off > 0; off >>= 1) {
    n_vis += __shfl_down(n_vis, off);
    n_pt += __shfl_down(n_pt, off);
  }
#ifdef RT_PHASE_TIMING
  for (int off = 32; off > 0; off >>= 1) ph_lane_steps += __shfl_down(ph_lane_steps, off);
  if (lane == 0) atomicAdd(&kblock(P.kconst)->counters[blockIdx.x % kCounterSlots].pad[kPhLaneSteps], ph_lane_steps);
#endif
  if (lane == 0) {
    DCounters* cs = kblock(P.kconst)->counters + (blockIdx.x % kCounterSlots);
    atomicAdd(&cs->segments, n_seg);
    atomicAdd(&cs->samples, n_samp);
    atomicAdd(&cs->node_visits, n_vis);
    atomicAdd(&cs->prim_tests, n_pt);
#ifdef RT_PHASE_TIMING
    for (int b = 0; b < kPhBuckets; ++b)
      if (b != kPhLaneSteps && b != kPhWaveSteps) atomicAdd(&cs->pad[b], ph_t[b]);
    atomicAdd(&cs->pad[kPhWaveSteps], ph_wave_steps);
#endif
  }
}

// Sum the per-chunk partials of each pixel in chunk order and write the Image.data layout
// (row 0 = bottom, image.rs:10-14) or the packed tile layout used by the multi-GPU gather.
// accumulate: a later sample pass of the same call — the sum starts from the value the earlier passes
// left in `out` and goes on adding chunks in order, so the additions are exactly one pass's.
__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ partial, int n_chunks,
                                                     int n_tiles_rank, int tiles_x, int ty0, int tile_rank,
                                                     int tile_world, int width, int row0, int row1, int packed,
                                                     int accumulate, double* __restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long n_pix = (long long)n_tiles_rank * kTilePixels;
  if (i >= n_pix) return;
  long long lt = i / kTilePixels;
  int lp = (int)(i % kTilePixels);
  long long gt = lt * tile_world + tile_rank;
  int px = (int)(gt % tiles_x) * kTile + lp % kTile;
  int py = (ty0 + (int)(gt / tiles_x)) * kTile + lp / kTile;
  bool inside = px < width && py >= row0 && py < row1;
  double r = 0.0, g = 0.0, b = 0.0;
  const long long o = packed ? i * 3 : ((long long)(py - row0) * width + px) * 3;
  if (accumulate && (packed || inside)) {
    r = out[o + 0];
    g = out[o + 1];
    b = out[o + 2];
  }
  if (inside) {
    // (unrolled: the loads of 8 chunks in flight at once — a sharded frame's reduce runs few waves per
    // CU over many chunks; the additions stay in chunk order)
#pragma unroll 8
    for (int c = 0; c < n_chunks; ++c) {
      const double* p = partial + ((long long)c * n_pix + i) * 3;
      r += p[0];
      g += p[1];
      b += p[2];
    }
  }
  if (packed || inside) {
    out[o + 0] = r;
    out[o + 1] = g;
    out[o + 2] = b;
  }
}

// The reduce of an adaptive step (rt_render_adaptive; adaptive.h): one wave per listed tile, one lane per
// pixel, so a 256-thread block serves four tiles.  The partials ([n_chunks][n_list * 64][3], one chunk =
// one batch) are read once.  Per in-image pixel, in chunk order: accum[c] += p[c] from the stored value —
// reduce_kernel's additions with `accumulate` — and the batch observation y = (p[0] + p[1]) + p[2] goes
// into the pixel's moments, m1 += y, m2 = fma(y, y, m2) ([H][W][2] f64).  Then the tile's error after
// n_batches batches per pixel: the lanes' variances and first moments are summed over the wave by an xor
// butterfly — offsets 32, 16, 8, 4, 2, 1, lane l adding lane l ^ offset's value to its own, so every lane
// holds the same sum of a fixed tree (no atomics) — and lane 0 writes tile_error(...) to err[list
// position].  Out-of-image lanes of edge tiles contribute 0 and are not counted in K.
__global__ __launch_bounds__(256) void fold_stats_kernel(const double* __restrict__ partial, int n_chunks, int n_list,
                                                         const uint32_t* __restrict__ tile_list, int tiles_x,
                                                         int width, int height, long long n_batches, int batch,
                                                         double noise_floor, double* __restrict__ accum,
                                                         double* __restrict__ moments, double* __restrict__ err) {
  const int lt = (int)(blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave);  // wave-uniform
  if (lt >= n_list) return;
  const int lp = (int)(threadIdx.x % kWave);
  const uint32_t g = tile_list[lt];
  const int px = (int)(g % (uint32_t)tiles_x) * kTile + lp % kTile;
  const int py = (int)(g / (uint32_t)tiles_x) * kTile + lp / kTile;
  const bool inside = px < width && py < height;
  double v = 0.0, m1 = 0.0;
  if (inside) {
    const long long pix = (long long)py * width + px;
    const long long n_pix = (long long)n_list * kTilePixels, i = (long long)lt * kTilePixels + lp;
    double r = accum[pix * 3 + 0], gr = accum[pix * 3 + 1], b = accum[pix * 3 + 2];
    double m2 = moments[pix * 2 + 1];
    m1 = moments[pix * 2 + 0];
#pragma unroll 8
    for (int c = 0; c < n_chunks; ++c) {
      const double* p = partial + ((long long)c * n_pix + i) * 3;
      const double p0 = p[0], p1 = p[1], p2 = p[2];
      r += p0;
      gr += p1;
      b += p2;
      const double y = (p0 + p1) + p2;
      m1 += y;
      m2 = fma(y, y, m2);
    }
    accum[pix * 3 + 0] = r;
    accum[pix * 3 + 1] = gr;
    accum[pix * 3 + 2] = b;
    moments[pix * 2 + 0] = m1;
    moments[pix * 2 + 1] = m2;
    v = pixel_variance(m1, m2, n_batches);
  }
  double E = v, M = inside ? m1 : 0.0;
  int K = inside ? 1 : 0;
  for (int off = kWave / 2; off > 0; off >>= 1) {
    E += __shfl_xor(E, off);
    M += __shfl_xor(M, off);
    K += __shfl_xor(K, off);
  }
  if (lp == 0) err[lt] = tile_error(E, M, K, n_batches, batch, noise_floor);
}

// rt_tonemap_counts_device: tonemap_kernel with the pixel's own sample count in place of the frame's
// (1 / count is the host's IEEE division too); a count of 0 gives black.
__global__ __launch_bounds__(256) void tonemap_counts_kernel(const double* __restrict__ accum,
                                                             const int32_t* __restrict__ counts, int width, int height,
                                                             uint8_t* __restrict__ rgb8) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n = (long long)width * height * 3;
  if (i >= n) return;
  const long long row = i / ((long long)width * 3), rest = i - row * width * 3;
  const long long src = ((long long)(height - 1 - row) * width) * 3 + rest;
  const int32_t cnt = counts[src / 3];
  if (cnt <= 0) {
    rgb8[i] = 0;
    return;
  }
  const double inv = 1.0 / (double)cnt;
  const double y = sqrt(accum[src] * inv) * 255.999;
  rgb8[i] = (y != y || y <= 0.0) ? (uint8_t)0 : (y >= 255.0 ? (uint8_t)255 : (uint8_t)y);
}

// Sample-partitioned frames (RT_PARTITION_SAMPLES): a rank's row band holds one partial band per rank,
// parts[r][i]; the band's sums are added in rank order (deterministic for any arrival order).
__global__ __launch_bounds__(256) void sum_parts_kernel(const double* __restrict__ parts, int n_parts, long long n,
                                                        double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = parts[i];
  for (int r = 1; r < n_parts; ++r) s += parts[(long long)r * n + i];
  out[i] = s;
}

// image.rs:31-44 to_image + color.rs:31-38 to_pixel on the device: per channel c * (1/S), sqrt,
// * 255.999 and Rust's saturating `as u8` (NaN -> 0); image row j becomes output row H-1-j.
// One thread per output byte (coalesced stores).
__global__ __launch_bounds__(256) void tonemap_kernel(const double* __restrict__ accum, int width, int height,
                                                      double inv, uint8_t* __restrict__ rgb8) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n = (long long)width * height * 3;
  if (i >= n) return;
  const long long row = i / ((long long)width * 3), rest = i - row * width * 3;
  const double y = sqrt(accum[((long long)(height - 1 - row) * width) * 3 + rest] * inv) * 255.999;
  rgb8[i] = (y != y || y <= 0.0) ? (uint8_t)0 : (y >= 255.0 ? (uint8_t)255 : (uint8_t)y);
}

// Scatter a gathered [world][max_tiles][64][3] buffer into the [H][W][3] image.
__global__ __launch_bounds__(256) void unpack_kernel(const double* __restrict__ gathered, int world, int max_tiles,
                                                     int n_tiles_total, int tiles_x, int width, int height,
                                                     double* __restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)world * max_tiles * kTilePixels;
  if (i >= total) return;
  int lp = (int)(i % kTilePixels);
  long long t = i / kTilePixels;
  int lt = (int)(t % max_tiles);
  int r = (int)(t / max_tiles);
  long long gt = (long long)lt * world + r;
  if (gt >= n_tiles_total) return;
  int px = (int)(gt % tiles_x) * kTile + lp % kTile;
  int py = (int)(gt / tiles_x) * kTile + lp / kTile;
  if (px >= width || py >= height) return;
  long long o = ((long long)py * width + px) * 3;
  out[o + 0] = gathered[i * 3 + 0];
  out[o + 1] = gathered[i * 3 + 1];
  out[o + 2] = gathered[i * 3 + 2];
}

// Closest hit for a batch of rays (rt_scene_hit): one lane per ray, same traversal + record code.
struct HitOut {
  int32_t object, front_face;
  double t, point[3], normal[3], u, v;
};
template <int MODE>
__global__ __launch_bounds__(kHitThreads) void hit_kernel(DScene S, const double* __restrict__ rays, int n,
                                                          double t_min, double t_max, HitOut* __restrict__ out) {
  extern __shared__ unsigned char lds_raw[];
  const int tid = threadIdx.x;
  DNode* lds_nodes = reinterpret_cast<DNode*>(lds_raw);
  unsigned char* stk_base = lds_raw + (size_t)S.n_lds_nodes * sizeof(DNode);
  int* stk_node = reinterpret_cast<int*>(stk_base) + tid;
  float* stk_t = reinterpret_cast<float*>(stk_base + (size_t)S.stack_depth * kHitThreads * 4) + tid;
  stage_nodes<MODE>(S, lds_nodes);
  int i = blockIdx.x * kHitThreads + tid;
  if (i >= n) return;
  v3 o = V(rays[i * 6 + 0], rays[i * 6 + 1], rays[i * 6 + 2]);
  v3 d = V(rays[i * 6 + 3], rays[i * 6 + 4], rays[i * 6 + 5]);
  double t_best = t_max;
  int face = -1;
  unsigned visits = 0, ptests = 0;
  // side-stream key of a free ray (book-2 media): pixel = ray index, sample 0, draw 0, seed 0
  const Rng rk{(uint32_t)i, 0u, 0u, 0u, 0u};
  int prim = traverse<kHitThreads, MODE, true>(S, lds_nodes, o, d, t_min, t_best, face, rk, 0ull, stk_node, stk_t, visits,
                                         ptests);
  HitOut r{};
  r.object = prim;
  if (prim >= 0) {
    const DPrim pr = S.prims[prim];
    Hit h;
    hit_record<true, true>(S, pr, face, o, d, t_best, rk, 0ull, h);
    r.front_face = h.front_face ? 1 : 0;
    r.t = h.t;
    r.point[0] = h.point.x; r.point[1] = h.point.y; r.point[2] = h.point.z;
    r.normal[0] = h.normal.x; r.normal[1] = h.normal.y; r.normal[2] = h.normal.z;
    r.u = h.u;
    r.v = h.v;
  }
  out[i] = r;
}

// Closest hit for a batch of rays through the traversal the renderer runs (rt_scene_hit_ex with
// RT_TRAVERSAL_RENDER): the 4-wide tree with conservative f32 (inflated) child boxes, exact f64 leaf
// re-tests and the f64 fallback for far origins (traverse4), with nodes / primitives read from the
// place trace_kernel reads them (MODE) and the trace kernel's EXT instance.  One lane per ray; the
// hit record is rebuilt like hit_kernel's.
template <int MODE, bool EXT>
__global__ __launch_bounds__(kHitThreads) void hit4_kernel(DScene S, const double* __restrict__ rays, int n,
                                                           double t_min, double t_max, HitOut* __restrict__ out) {
  extern __shared__ unsigned char lds_raw[];
  const int tid = threadIdx.x;
  typedef typename Node4Sel<EXT>::T N4;
  const BlockLds<N4> L = carve_block_lds<MODE, N4>(S, lds_raw);
  stage_nodes4<MODE>(S, L.nodes, L.prims);
  const int i = blockIdx.x * kHitThreads + tid;
  if (i >= n) return;
  const v3 o = V(rays[i * 6 + 0], rays[i * 6 + 1], rays[i * 6 + 2]);
  const v3 d = V(rays[i * 6 + 3], rays[i * 6 + 4], rays[i * 6 + 5]);
  double t_best = t_max;
  int face = -1;
  unsigned visits = 0, ptests = 0;
  const Rng rk{(uint32_t)i, 0u, 0u, 0u, 0u};  // side-stream key of a free ray, as hit_kernel's
#ifdef RT_PHASE_TIMING
  unsigned long long steps = 0;
#endif
  const int prim = traverse4<kHitThreads, MODE, EXT>(S, L.nodes, L.prims, o, d, t_min, t_best, face, L.stk, rk, 0ull,
                                                      visits, ptests RT_STAT_ARG(steps));
  HitOut r{};
  r.object = prim;
  if (prim >= 0) {
    const DPrim pr = S.prims[prim];
    Hit h;
    hit_record<true, true>(S, pr, face, o, d, t_best, rk, 0ull, h);
    r.front_face = h.front_face ? 1 : 0;
    r.t = h.t;
    r.point[0] = h.point.x; r.point[1] = h.point.y; r.point[2] = h.point.z;
    r.normal[0] = h.normal.x; r.normal[1] = h.normal.y; r.normal[2] = h.normal.z;
    r.u = h.u;
    r.v = h.v;
  }
  out[i] = r;
}

// rt_probe_segment: one ray_color iteration (render.rs:30-46) per given ray through trace_kernel's own
// steps 1, 3 and 4 for a lane that holds a path — the render traversal, the hit record, the material and
// its texture leaf, the wave's marble and sampler, the one normalisation, shade_factor (or the sky) — on
// the path key (seed, pixel = ray index, sample, draw).  Lanes past n take part in the wave-wide steps
// idle, like a megakernel lane without a path.
struct ProbeOut {
  int32_t object, front_face, scattered, emits;
  uint32_t draw;
  int32_t pad;
  double t, point[3], normal[3], emitted[3], attenuation[3], origin[3], direction[3];
};
static_assert(sizeof(ProbeOut) == 176, "ProbeOut is rt_probe (include/shirley_rt.h)");
template <int MODE, bool EXT>
__global__ __launch_bounds__(kHitThreads) void probe_kernel(DScene S, const double* __restrict__ rays, int n,
                                                            uint64_t seed, uint32_t sample, uint32_t draw0,
                                                            ProbeOut* __restrict__ out) {
  extern __shared__ unsigned char lds_raw[];
  const int tid = threadIdx.x;
  typedef typename Node4Sel<EXT>::T N4;
  const BlockLds<N4> L = carve_block_lds<MODE, N4>(S, lds_raw);
  stage_nodes4<MODE>(S, L.nodes, L.prims);
  const int i = blockIdx.x * kHitThreads + tid;
  const bool active = i < n;
  v3 o = V(0.0, 0.0, 0.0), d = V(1.0, 1.0, 1.0);
  if (active) {
    o = V(rays[i * 6 + 0], rays[i * 6 + 1], rays[i * 6 + 2]);
    d = V(rays[i * 6 + 3], rays[i * 6 + 4], rays[i * 6 + 5]);
  }
  Rng rng{(uint32_t)i, sample, draw0, 0u, 0u};
  if (draw0 & 1u) {  // an odd counter reads the odd half of block draw0 / 2 from the cache
    uint64_t e0, e1;
    philox_block(seed, rng.pixel, rng.sample, draw0 >> 1, e0, e1);
    rng.c2 = (uint32_t)e1;
    rng.c3 = (uint32_t)(e1 >> 32);
  }
  unsigned visits = 0, ptests = 0;
#ifdef RT_PHASE_TIMING
  unsigned long long steps = 0;
#endif
  // step 1 (trace_kernel): closest hit, record, material, texture leaf
  bool hit = false, need_pn = false, need_r = false;
  int prim = -1, face = -1, leaf = -1, mat = 0, ptab = 0, mk = -1;
  double t_best = __builtin_inf(), psc = 0.0;
  Hit h;
  h.point = V(0.0, 0.0, 0.0);
  h.normal = h.point;
  h.t = h.u = h.v = 0.0;
  h.front_face = false;
  if (active) {
    prim = traverse4<kHitThreads, MODE, EXT>(S, L.nodes, L.prims, o, d, 0.001, t_best, face, L.stk, rng, seed, visits,
                                              ptests RT_STAT_ARG(steps));
    if (prim >= 0) {
      hit = true;
      const DPrim pr = (MODE == kSceneLds) ? L.prims[prim] : S.prims[prim];
      hit_record<false, EXT>(S, pr, face, o, d, t_best, rng, seed, h);
      mat = pr.material;
      mk = S.mats[mat].kind;
      need_r = mk == RT_MAT_LAMBERTIAN || mk == RT_MAT_METAL || mk == RT_MAT_FAIRY_LIGHT || mk == RT_MAT_ISOTROPIC;
      if (mk == RT_MAT_LAMBERTIAN || mk == RT_MAT_FAIRY_LIGHT || mk == RT_MAT_DIFFUSE_LIGHT || mk == RT_MAT_ISOTROPIC)
        leaf = texture_leaf(S, S.mats[mat].tex, h.point, need_pn, ptab, psc);
    }
  }
  const bool ends = active && (!hit || mk == RT_MAT_DIFFUSE_LIGHT);
  // step 3: the wave's marble values and draws
  const double pn = wave_marble(S, L.perlin, need_pn, ptab, psc, h.point);
  const bool scat = active && !ends;
  const int dk = (scat && need_r) ? kDrawSphere : (scat && mk == RT_MAT_DIELECTRIC) ? kDrawDiel : kDrawNone;
  double jx = 0.0, jy = 0.0;
  const v3 rs = draws_coop(rng, seed, dk, false, 0u, jx, jy);
  const v3 un = unit_fast(!active ? V(1.0, 1.0, 1.0) : (scat && need_r && mk != RT_MAT_METAL) ? rs : d);
  // step 4: emitted + scatter, or the sky
  if (!active) return;
  ProbeOut r{};
  r.object = prim;
  bool alive = false, has_emit = false;
  v3 mul = V(1.0, 1.0, 1.0), emit = V(0.0, 0.0, 0.0);
  if (hit) {
    const DMat& m = S.mats[mat];
    alive = shade_factor(S, S.texs, m, leaf, pn, rs, un, rng, o, d, h, prim, face, mul, emit, has_emit);
    r.front_face = h.front_face ? 1 : 0;
    r.t = h.t;
    r.point[0] = h.point.x; r.point[1] = h.point.y; r.point[2] = h.point.z;
    r.normal[0] = h.normal.x; r.normal[1] = h.normal.y; r.normal[2] = h.normal.z;
  } else {
    emit = sky_unit(S, un);
    has_emit = true;
  }
  r.scattered = alive ? 1 : 0;
  r.emits = has_emit ? 1 : 0;
  r.draw = rng.draw;
  r.emitted[0] = emit.x; r.emitted[1] = emit.y; r.emitted[2] = emit.z;
  if (alive) {
    r.attenuation[0] = mul.x; r.attenuation[1] = mul.y; r.attenuation[2] = mul.z;
    r.origin[0] = o.x; r.origin[1] = o.y; r.origin[2] = o.z;
    r.direction[0] = d.x; r.direction[1] = d.y; r.direction[2] = d.z;
  }
  out[i] = r;
}

// ------------------------------------------------------------------------------------------
// launch wrappers (declared in rt_launch.h, called from rt_api.cpp)
// ------------------------------------------------------------------------------------------
// (megakernel block LDS: trace_lds_bytes, rt_layout.h)
size_t hit_lds_bytes(int n_lds_nodes, int stack_depth) { return lds_bytes(n_lds_nodes, stack_depth, kHitThreads); }

static int node_mode(const DScene& S) {
  return S.n_lds_nodes >= S.n_nodes ? kNodesLds : (S.n_lds_nodes == 0 ? kNodesGlobal : kNodesMixed);
}

template <int THREADS, int MODE, bool EXT, int HOP = 0>
static hipError_t occupancy_impl1(const DScene& S, int* blocks_per_cu) {
  // allow dynamic LDS beyond the 64 KiB default (gfx950 has 160 KiB per CU)
  const size_t lds = trace_lds_bytes(S.n_lds_nodes4, node4_bytes(S.exts != nullptr), S.n_lds_prims, S.n_lds_perlin, S.stack_depth4, THREADS,
                                     S.n_lds_mats, S.n_lds_texs);
  hipError_t e = hipFuncSetAttribute((const void*)trace_kernel<THREADS, MODE, EXT, false, HOP>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  // (the tile-list instance runs in the same launch shape: same block, same LDS)
  e = hipFuncSetAttribute((const void*)trace_kernel<THREADS, MODE, EXT, true, HOP>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, trace_kernel<THREADS, MODE, EXT, false, HOP>, THREADS,
                                                      lds);
}
template <int THREADS, int MODE>
static hipError_t occupancy_impl(const DScene& S, int* blocks_per_cu) {
  return S.exts ? occupancy_impl1<THREADS, MODE, true>(S, blocks_per_cu)
                : occupancy_impl1<THREADS, MODE, false>(S, blocks_per_cu);
}
template <int THREADS, int MODE, bool EXT, int HOP = 0>
static void launch_trace2(const KParams& p, int blocks, size_t lds, hipStream_t stream) {
  if (p.work.tile_list)
    hipLaunchKernelGGL((trace_kernel<THREADS, MODE, EXT, true, HOP>), dim3(blocks), dim3(THREADS), lds, stream, p);
  else
    hipLaunchKernelGGL((trace_kernel<THREADS, MODE, EXT, false, HOP>), dim3(blocks), dim3(THREADS), lds, stream, p);
}
template <int THREADS, int MODE>
static void launch_trace1(const KParams& p, int blocks, size_t lds, hipStream_t stream) {
  if (p.scene.exts)
    launch_trace2<THREADS, MODE, true>(p, blocks, lds, stream);
  else
    launch_trace2<THREADS, MODE, false>(p, blocks, lds, stream);
}

static hipError_t hit_prepare(const DScene& S) {
  const int lds = (int)hit_lds_bytes(S.n_lds_nodes, S.stack_depth);
  switch (node_mode(S)) {
    case kNodesLds: return hipFuncSetAttribute((const void*)hit_kernel<kNodesLds>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    case kNodesGlobal: return hipFuncSetAttribute((const void*)hit_kernel<kNodesGlobal>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    default: return hipFuncSetAttribute((const void*)hit_kernel<kNodesMixed>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  }
}

// Kernel instances: the wide block only with the whole (4-wide) BVH in LDS.  Also prepares the
// rt_scene_hit kernel for the scene.  `hop` (scene_compile.h hop_instance): the scene-in-LDS reference-scene instances
// with the hop pass; an error for a scene that runs any other instance.
hipError_t trace_occupancy(const DScene& S, int threads, int hop, int* blocks_per_cu) {
  hipError_t e = hit_prepare(S);
  if (e != hipSuccess) return e;
  if (hop && !(threads == kTraceThreadsWide && !S.exts && S.n_lds_prims > 0)) return hipErrorInvalidValue;
  if (threads == kTraceThreadsWide && !S.exts) {  // reference scenes only: book-2 scenes take kTraceThreadsWide3
    if (node_mode4(S) != kNodesLds) return hipErrorInvalidValue;
    if (hop == 4) return occupancy_impl1<kTraceThreadsWide, kSceneLds, false, 4>(S, blocks_per_cu);
    if (hop == 3) return occupancy_impl1<kTraceThreadsWide, kSceneLds, false, 3>(S, blocks_per_cu);
    if (hop == 2) return occupancy_impl1<kTraceThreadsWide, kSceneLds, false, 2>(S, blocks_per_cu);
    if (hop) return occupancy_impl1<kTraceThreadsWide, kSceneLds, false, 1>(S, blocks_per_cu);
    if (S.n_lds_prims > 0) return occupancy_impl1<kTraceThreadsWide, kSceneLds, false>(S, blocks_per_cu);
    return occupancy_impl1<kTraceThreadsWide, kNodesLds, false>(S, blocks_per_cu);
  }
  if (threads == kTraceThreadsWide3) {  // book-2 scenes only (scene_compile.cpp)
    if (node_mode4(S) != kNodesLds || !S.exts) return hipErrorInvalidValue;
    if (S.n_lds_prims > 0) return occupancy_impl1<kTraceThreadsWide3, kSceneLds, true>(S, blocks_per_cu);
    return occupancy_impl1<kTraceThreadsWide3, kNodesLds, true>(S, blocks_per_cu);
  }
  switch (node_mode4(S)) {
    case kNodesLds: return occupancy_impl<kTraceThreads, kNodesLds>(S, blocks_per_cu);
    case kNodesGlobal: return occupancy_impl<kTraceThreads, kNodesGlobal>(S, blocks_per_cu);
    default: return occupancy_impl<kTraceThreads, kNodesMixed>(S, blocks_per_cu);
  }
}

hipError_t launch_trace(const KParams& p, int blocks, int threads, int hop, hipStream_t stream) {
  const size_t lds = trace_lds_bytes(p.scene.n_lds_nodes4, node4_bytes(p.scene.exts != nullptr), p.scene.n_lds_prims, p.scene.n_lds_perlin, p.scene.stack_depth4, threads,
                                     p.scene.n_lds_mats, p.scene.n_lds_texs);
  if (hop && !(threads == kTraceThreadsWide && !p.scene.exts && p.scene.n_lds_prims > 0)) return hipErrorInvalidValue;
  if (threads == kTraceThreadsWide && !p.scene.exts) {
    if (hop == 4)
      launch_trace2<kTraceThreadsWide, kSceneLds, false, 4>(p, blocks, lds, stream);
    else if (hop == 3)
      launch_trace2<kTraceThreadsWide, kSceneLds, false, 3>(p, blocks, lds, stream);
    else if (hop == 2)
      launch_trace2<kTraceThreadsWide, kSceneLds, false, 2>(p, blocks, lds, stream);
    else if (hop)
      launch_trace2<kTraceThreadsWide, kSceneLds, false, 1>(p, blocks, lds, stream);
    else if (p.scene.n_lds_prims > 0)
      launch_trace2<kTraceThreadsWide, kSceneLds, false>(p, blocks, lds, stream);
    else
      launch_trace2<kTraceThreadsWide, kNodesLds, false>(p, blocks, lds, stream);
    return hipGetLastError();
  }
  if (threads == kTraceThreadsWide3) {
    if (!p.scene.exts) return hipErrorInvalidValue;
    if (p.scene.n_lds_prims > 0)
      launch_trace2<kTraceThreadsWide3, kSceneLds, true>(p, blocks, lds, stream);
    else
      launch_trace2<kTraceThreadsWide3, kNodesLds, true>(p, blocks, lds, stream);
    return hipGetLastError();
  }
  switch (node_mode4(p.scene)) {
    case kNodesLds: launch_trace1<kTraceThreads, kNodesLds>(p, blocks, lds, stream); break;
    case kNodesGlobal: launch_trace1<kTraceThreads, kNodesGlobal>(p, blocks, lds, stream); break;
    default: launch_trace1<kTraceThreads, kNodesMixed>(p, blocks, lds, stream);
  }
  return hipGetLastError();
}

hipError_t launch_hit(const DScene& S, const double* rays, int n, double t_min, double t_max, void* out,
                      hipStream_t stream) {
  int blocks = (n + kHitThreads - 1) / kHitThreads;
  if (blocks == 0) return hipSuccess;
  size_t lds = hit_lds_bytes(S.n_lds_nodes, S.stack_depth);
  HitOut* o = static_cast<HitOut*>(out);
  switch (node_mode(S)) {
    case kNodesLds: hipLaunchKernelGGL(hit_kernel<kNodesLds>, dim3(blocks), dim3(kHitThreads), lds, stream, S, rays, n, t_min, t_max, o); break;
    case kNodesGlobal: hipLaunchKernelGGL(hit_kernel<kNodesGlobal>, dim3(blocks), dim3(kHitThreads), lds, stream, S, rays, n, t_min, t_max, o); break;
    default: hipLaunchKernelGGL(hit_kernel<kNodesMixed>, dim3(blocks), dim3(kHitThreads), lds, stream, S, rays, n, t_min, t_max, o);
  }
  return hipGetLastError();
}

// rt_scene_hit_ex(RT_TRAVERSAL_RENDER): the node / primitive placement the trace kernel uses (pass_frame.h
// dispatch_placement; the block is kHitThreads on every placement) and the trace kernel's EXT instance.
hipError_t launch_hit4(const DScene& S, bool wide, const double* rays, int n, double t_min, double t_max, void* out,
                       hipStream_t stream) {
  const int blocks = (n + kHitThreads - 1) / kHitThreads;
  if (blocks == 0) return hipSuccess;
  HitOut* o = static_cast<HitOut*>(out);
  return dispatch_placement<kHitThreads>(S, wide, [&](auto, auto mode) {
    constexpr int M = decltype(mode)::value;
    auto go = [&](auto kernel, bool ext) {
      return launch_block(kernel, blocks, kHitThreads, block_lds_bytes<M>(S, node4_bytes(ext), kHitThreads), stream, S,
                          rays, n, t_min, t_max, o);
    };
    return S.exts ? go(hit4_kernel<M, true>, true) : go(hit4_kernel<M, false>, false);
  });
}

// rt_probe_segment: placed as launch_hit4
hipError_t launch_probe(const DScene& S, bool wide, const double* rays, int n, uint64_t seed, uint32_t sample,
                        uint32_t draw, void* out, hipStream_t stream) {
  const int blocks = (n + kHitThreads - 1) / kHitThreads;
  if (blocks == 0) return hipSuccess;
  ProbeOut* o = static_cast<ProbeOut*>(out);
  return dispatch_placement<kHitThreads>(S, wide, [&](auto, auto mode) {
    constexpr int M = decltype(mode)::value;
    auto go = [&](auto kernel, bool ext) {
      return launch_block(kernel, blocks, kHitThreads, block_lds_bytes<M>(S, node4_bytes(ext), kHitThreads), stream, S,
                          rays, n, seed, sample, draw, o);
    };
    return S.exts ? go(probe_kernel<M, true>, true) : go(probe_kernel<M, false>, false);
  });
}

hipError_t launch_reduce(const double* partial, int n_chunks, int n_tiles_rank, int tiles_x, int ty0, int tile_rank,
                         int tile_world, int width, int row0, int row1, int packed, int accumulate, double* out,
                         hipStream_t stream) {
  long long n = (long long)n_tiles_rank * kTilePixels;
  int blocks = (int)((n + 255) / 256);
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(reduce_kernel, dim3(blocks), dim3(256), 0, stream, partial, n_chunks, n_tiles_rank, tiles_x,
                     ty0, tile_rank, tile_world, width, row0, row1, packed, accumulate, out);
  return hipGetLastError();
}

hipError_t launch_fold_stats(const double* partial, int n_chunks, int n_list, const uint32_t* tile_list, int tiles_x,
                             int width, int height, long long n_batches, int batch, double noise_floor,
                             double* accum, double* moments, double* err, hipStream_t stream) {
  const int blocks = (n_list + 3) / 4;  // one wave per listed tile
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(fold_stats_kernel, dim3(blocks), dim3(256), 0, stream, partial, n_chunks, n_list, tile_list,
                     tiles_x, width, height, n_batches, batch, noise_floor, accum, moments, err);
  return hipGetLastError();
}

hipError_t launch_tonemap_counts(const double* accum, const int32_t* counts, int width, int height, uint8_t* rgb8,
                                 hipStream_t stream) {
  const long long n = (long long)width * height * 3;
  const int blocks = (int)((n + 255) / 256);
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(tonemap_counts_kernel, dim3(blocks), dim3(256), 0, stream, accum, counts, width, height, rgb8);
  return hipGetLastError();
}

hipError_t launch_sum_parts(const double* parts, int n_parts, long long n, double* out, hipStream_t stream) {
  const long long blocks = (n + 255) / 256;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, parts, n_parts, n, out);
  return hipGetLastError();
}

#ifdef RT_TIMELINE
// timeline build: per-wave exit times of the last launch relative to the first wave's start, and each
// wave's time from seeing the unit pool exhausted to its exit (the frame's tail)
void timeline_dump() {
  {
    static unsigned long long t0[kTimelineWaves], tx[kTimelineWaves], t1[kTimelineWaves];
    if (hipMemcpyFromSymbol(t0, HIP_SYMBOL(g_wave_t0), sizeof t0) == hipSuccess &&
        hipMemcpyFromSymbol(tx, HIP_SYMBOL(g_wave_tx), sizeof tx) == hipSuccess &&
        hipMemcpyFromSymbol(t1, HIP_SYMBOL(g_wave_t1), sizeof t1) == hipSuccess) {
      std::vector<double> ends, tails, firstx;
      unsigned long long tmin = ~0ull;
      for (int i = 0; i < kTimelineWaves; ++i)
        if (t1[i] && t0[i]) tmin = std::min(tmin, t0[i]);
      for (int i = 0; i < kTimelineWaves; ++i)
        if (t1[i] && t0[i] && t1[i] >= tmin) {
          ends.push_back((double)(t1[i] - tmin) * 1e-2);  // 100 MHz ticks -> us
          if (tx[i] && tx[i] <= t1[i]) {
            tails.push_back((double)(t1[i] - tx[i]) * 1e-2);
            firstx.push_back((double)(tx[i] - tmin) * 1e-2);
          }
        }
      auto pct = [](std::vector<double> v, double q) {
        if (v.empty()) return 0.0;
        std::sort(v.begin(), v.end());
        return v[std::min(v.size() - 1, (size_t)(q * (double)(v.size() - 1)))];
      };
      fprintf(stderr, "[phase-timeline] waves %zu; exit us p0 %.1f p50 %.1f p90 %.1f p99 %.1f p99.9 %.1f max %.1f; "
              "pool exhausted seen at us p0 %.1f p50 %.1f; exhausted->exit us p50 %.1f p90 %.1f p99 %.1f max %.1f\n",
              ends.size(), pct(ends, 0), pct(ends, 0.5), pct(ends, 0.9), pct(ends, 0.99), pct(ends, 0.999),
              pct(ends, 1), pct(firstx, 0), pct(firstx, 0.5), pct(tails, 0.5), pct(tails, 0.9), pct(tails, 0.99),
              pct(tails, 1));
      std::fill(t0, t0 + kTimelineWaves, 0ull);
      (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wave_t0), t0, sizeof t0);
      (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wave_tx), t0, sizeof t0);
      (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wave_t1), t0, sizeof t0);
    }
  }
}
#endif

#ifdef RT_PHASE_TIMING
// instrumented build: print and clear the event counters (slot 2i: lane events, 2i + 1: wave events)
void phase_counters_dump() {
  unsigned long long h[2 * kPhaseEvents];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase_ctr), sizeof h) != hipSuccess) return;
  static const char* names[] = {"visit", "visit_with_leaves", "sphere_iter", "sphere_slab_pass", "rect_iter",
                                "pop_iter", "segment_iter", "box_iter", "marble_round", "draws_coop_round",
                                "unit_fetch", "camera_ray", "philox_A", "philox_B", "marble_sin", "hit_record",
                                "checker_level", "dielectric", "metal", "lambertian", "sky", "diffuse_light",
                                "reflectance", "traverse4", "publish", "tie_resolve", "hop_candidate", "hop_served",
                                "hop2_candidate", "hop2_served", "hop_guarded",
                                // lanes whose traversal hit is a dielectric primitive of the ground stack, and those
                                // of them in wave-iterations that hold at least 8 / 16 / 24 / 32 such lanes
                                "down_hit", "down_hit_ge8", "down_hit_ge16", "down_hit_ge24", "down_hit_ge32",
                                // the down pass (HOP = 3), per run: lanes tried, served, found, left waiting
                                "down1_try", "down1_served", "down1_found", "down1_wait",
                                "down2_try", "down2_served", "down2_found", "down2_wait",
                                "down3_try", "down3_served", "down3_found", "down3_wait",
                                // ... and the lanes of each run that ask the stack (alive, running inward or down):
                                // ask - served - found were refused (HOP = 4: declined)
                                "down1_ask", "down2_ask", "down3_ask",
                                // HOP = 4: the serve body's lanes by form, in the down pass and in step 5'
                                "down_serve_y", "down_serve_general", "hop_serve_y", "hop_serve_general"};
  static_assert(sizeof names / sizeof names[0] <= kPhaseEvents, "event slots");
  for (int i = 0; i < (int)(sizeof names / sizeof names[0]); ++i)
    if (h[2 * i + 1])
      fprintf(stderr, "[phase-ev] %-18s lanes %.4g waves %.4g lanes/wave %.2f\n", names[i], (double)h[2 * i],
              (double)h[2 * i + 1], (double)h[2 * i] / (double)h[2 * i + 1]);
  unsigned long long lh[64], wh[64];
  if (hipMemcpyFromSymbol(lh, HIP_SYMBOL(g_visit_hist), sizeof lh) == hipSuccess &&
      hipMemcpyFromSymbol(wh, HIP_SYMBOL(g_wave_visit_hist), sizeof wh) == hipSuccess) {
    fprintf(stderr, "[phase-hist] visits: lanes / waves (slowest lane)\n");
    for (int i = 1; i < 64; ++i)
      if (lh[i] || wh[i]) fprintf(stderr, "[phase-hist] %2d %.6g %.6g\n", i, (double)lh[i], (double)wh[i]);
  }
  unsigned long long hc[kHopClks];
  if (hipMemcpyFromSymbol(hc, HIP_SYMBOL(g_hop_clk), sizeof hc) == hipSuccess) {
    // (per run: the waves of down1_try + down2_try + down3_try, hop_candidate + hop2_candidate, hop_served + hop2_served)
    const double down_runs = (double)(h[2 * 36 + 1] + h[2 * 40 + 1] + h[2 * 44 + 1]);
    const double hop_runs = (double)(h[2 * 26 + 1] + h[2 * 28 + 1]), hop_serves = (double)(h[2 * 27 + 1] + h[2 * 29 + 1]);
    fprintf(stderr, "[phase-run] down pass: runs %.4g, wave-cycles per run: serve body %.1f, next hit (+ guard) %.1f\n", down_runs,
            down_runs ? (double)hc[kHopClkDownServe] / down_runs : 0.0, down_runs ? (double)hc[kHopClkDownNext] / down_runs : 0.0);
    fprintf(stderr, "[phase-run] hop pass: runs %.4g, wave-cycles per run: next hit (+ guard) %.1f; serving runs %.4g, serve body %.1f\n",
            hop_runs, hop_runs ? (double)hc[kHopClkHopNext] / hop_runs : 0.0, hop_serves,
            hop_serves ? (double)hc[kHopClkHopServe] / hop_serves : 0.0);
    fprintf(stderr, "[phase-run] wave-cycles in all: down serve %.4g, down next %.4g, hop next %.4g, hop serve %.4g\n", (double)hc[0],
            (double)hc[1], (double)hc[2], (double)hc[3]);
    fprintf(stderr, "[phase-run] leaf_tests4 wave-cycles in all: RectBox loop %.4g, rect loop %.4g\n", (double)hc[kLeafClkBox],
            (double)hc[kLeafClkRect]);
    unsigned long long zc[kHopClks] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_hop_clk), zc, sizeof zc);
  }
  unsigned long long z[2 * kPhaseEvents] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_phase_ctr), z, sizeof z);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_visit_hist), z, 64 * sizeof z[0]);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wave_visit_hist), z, 64 * sizeof z[0]);
}
#endif

hipError_t launch_tonemap(const double* accum, int width, int height, double inv, uint8_t* rgb8, hipStream_t stream) {
  const long long n = (long long)width * height * 3;
  const int blocks = (int)((n + 255) / 256);
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(tonemap_kernel, dim3(blocks), dim3(256), 0, stream, accum, width, height, inv, rgb8);
  return hipGetLastError();
}

hipError_t launch_unpack(const double* gathered, int world, int max_tiles, int n_tiles_total, int tiles_x, int width,
                         int height, double* out, hipStream_t stream) {
  long long n = (long long)world * max_tiles * kTilePixels;
  int blocks = (int)((n + 255) / 256);
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(unpack_kernel, dim3(blocks), dim3(256), 0, stream, gathered, world, max_tiles, n_tiles_total,
                     tiles_x, width, height, out);
  return hipGetLastError();
}

}  // namespace rt
