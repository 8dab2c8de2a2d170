// scene_compile.h — scene compilation: an rt_scene_desc in, the device tables and the placement plan out.
//
// Pure host C++ (no HIP): validation, the digest, flattening of rotated sphere instances, the BBox tree and
// its 2- and 4-wide flattenings, the DPrim / DExt / DMat / DTex / DPerlin tables, and the decision where a
// block keeps what (ScenePlacement).  rt_scene_upload (rt_api.cpp) copies the result to the device and asks
// the runtime for the occupancies; tools/scene_plan.cpp prints it for tests/test_scene_plan.py.
#pragma once

#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "../../../include/shirley_rt.h"
#include "bvh_build.h"
#include "rt_layout.h"

namespace rt {

// The placement bits of rt_scene_upload's `bvh_builder` argument (the rest is the builder).
constexpr int32_t kPlacementMask = RT_BVH_NODES_GLOBAL | RT_BVH_NODES_HALF_LDS | RT_BVH_NODES_LDS;

// The upload-time tuning variables (tuning_from_env): names and meanings at their uses in scene_compile.cpp.
struct SceneTuning {
  int collapse_dp = -1;         // SHIRLEY_COLLAPSE_DP: 1 / 0 = always / never the optimal collapse (-1: per scene)
  bool has_lds_nodes = false;   // SHIRLEY_LDS_NODES=<k>: at most k nodes in LDS where no placement flag decides
  long long lds_nodes = 0;
  bool no_wide = false;         // SHIRLEY_NO_WIDE
  bool no_lds_prims = false;    // SHIRLEY_NO_LDS_PRIMS
  bool no_lds_mats = false;     // SHIRLEY_NO_LDS_MATS
  bool no_lds_perlin = false;   // SHIRLEY_NO_LDS_PERLIN
  bool no_hop = false;          // SHIRLEY_NO_HOP
  bool hop_root = false;        // SHIRLEY_HOP=root: the first-node hop pass where the ground-stack one would run
  bool hop_up = false;          // SHIRLEY_HOP=up: the ground-stack pass without its down pass (ScenePlacement.hop_down)
  bool hop_general = false;     // SHIRLEY_HOP=general: a plane stack keeps the general passes (ScenePlacement.hop_planes)
  double sah_box_weight = 4.0;  // SHIRLEY_SAH_BOXW=<c>
  bool sah_binned = false;      // SHIRLEY_SAH_BINNED
  bool wf_extend2 = false;      // SHIRLEY_WF_EXTEND2
  int split_nt = 8;             // SHIRLEY_SPLIT_NT
  int split_refill = 0;         // SHIRLEY_SPLIT_REFILL (>= 1; 0: not set, the context keeps its value)
};
// Reads the environment anew at every call (nothing is cached: a process may change it between uploads).
SceneTuning tuning_from_env();

// Everything decided about a scene's launches before the runtime is asked for occupancies.
struct ScenePlacement {
  bool wide = false;            // the megakernel keeps the whole 4-wide tree in LDS, one wide block per CU
  int mk_threads = kTraceThreads;  // its block: kTraceThreadsWide / kTraceThreadsWide3 (book-2) when wide
  bool collapse_dp = false;     // nodes4 is the optimal collapse (Collapse4), not the greedy one
  int32_t n_lds_nodes = 0, n_lds_nodes4 = 0, n_lds_prims = 0, n_lds_perlin = 0, n_lds_mats = 0, n_lds_texs = 0;
  int32_t stack_depth = 0, stack_depth4 = 0, root4 = 0;
  long long stack_bytes = 0;    // the 2-wide traversal stacks of a kTraceThreads block
  uint32_t key_mask = 0;
  float origin_limit = 0.f;
  int32_t wf_n_lds_nodes = 0;   // DScene.n_lds_nodes of the wavefront engine's scene (wf_extend block)
  bool wf_extend4 = false;      // eligible for the 4-wide scene-in-LDS extend kernel (wf_prepare4 decides)
  int split_nt = 0;             // RT_ENGINE_SPLIT: traversal waves per block to try (0: scene not eligible)
  int split_refill = 0;         // SceneTuning.split_refill
  bool hop_pass = false;        // the megakernel runs its instances with the hop pass (trace.hip)
  int hop_kind = 0;             // ... of which kind (rt_scene_stats.hop_kind): 1 first-node visit, 2 ground stack
  bool hop_down = false;        // hop_kind 2 with the down pass before the sampler (trace.hip, HOP = 3)
  bool hop_planes = false;      // hop_down on a plane stack: both passes by the closed-form next plane (HOP = 4)
};

// The megakernel's HOP instance of a placement (rt_launch.h launch_trace, trace_occupancy; rt_scene_hop_instance):
// hop_kind, or 3 for the ground-stack pass with the down pass, or 4 for the two on a plane stack.
inline int hop_instance(const ScenePlacement& P) {
  return P.hop_kind == 2 && P.hop_down ? (P.hop_planes ? 4 : 3) : P.hop_kind;
}

// The plan's fields of the megakernel's device scene record.
inline void place_scene(const ScenePlacement& P, DScene& S) {
  S.stack_depth = P.stack_depth;
  S.stack_depth4 = P.stack_depth4;
  S.root4 = P.root4;
  S.key_mask = P.key_mask;
  S.origin_limit = P.origin_limit;
  S.n_lds_nodes = P.n_lds_nodes;
  S.n_lds_nodes4 = P.n_lds_nodes4;
  S.n_lds_prims = P.n_lds_prims;
  S.n_lds_perlin = P.n_lds_perlin;
  S.n_lds_mats = P.n_lds_mats;
  S.n_lds_texs = P.n_lds_texs;
}

// The scene's light list (rt_scene_lights; include/shirley_rt.h has the listing rule): the public records in
// object order, the device copy of each (the same order) and the count of emitters the rule leaves out.
struct LightList {
  std::vector<rt_light> lights;
  std::vector<DLight> dev;
  int32_t n_unlisted = 0;
};
// Of a validated description.
LightList list_lights(const rt_scene_desc* d);

// The light grid of a light list (rt_scene_light_pick / rt_light_grid_host; include/shirley_rt.h has the build,
// operation for operation): the public record and the rows, cell (iz * n[1] + iy) * n[0] + ix first to last.
constexpr double kLightPickWeighted = 0.875;  // the share of a row that follows the weights w_j / W ...
constexpr double kLightPickUniform = 0.125;   // ... and the share spread evenly, which keeps every p_j > 0
constexpr int32_t kLightGridMaxCells = 64;
constexpr int64_t kLightGridMaxEntries = (int64_t)1 << 22;
struct LightGridTable {
  rt_light_grid info{};
  std::vector<double> cdf;  // n[0] * n[1] * n[2] rows of n_lights; stays empty when want_cdf is false
};
// RT_OK, or RT_E_INVALID for cells outside 1 ... 64 or a table of more than 2^22 entries.  No light: RT_OK, all
// of `info` zero, no row.
// `masks` (may be null; [cells][L] words of `rays` bits, rt_scene_light_visibility): the rows then follow the
// visibility-weighted rule of the header; without them the call is rt_scene_light_pick's, bit for bit.
int build_light_grid(const LightList& l, int32_t cells, bool want_cdf, LightGridTable* out,
                     const uint32_t* masks = nullptr, int32_t rays = 0);

// The path's draw `draw` of (seed, pixel, sample) on the host: the device's rng_next on Rng{pixel, sample, draw}.
double path_draw(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t draw);
// Ray i of (cell, light) in the grid `g` (rt_scene_light_visibility; include/shirley_rt.h): x[3] the cell point,
// w[3] the vector to the light's target (0 from inside a sphere light); true when the ray is traced, false when
// the bit is set without one.
bool light_visibility_ray(const rt_light_grid& g, const DLight& q, uint64_t seed, uint32_t cell, uint32_t light,
                          uint32_t i, double* x, double* w);
inline bool light_visibility_rays_ok(int32_t rays) {
  return rays == 1 || rays == 2 || rays == 4 || rays == 8 || rays == 16 || rays == 32;
}

// What rt_scene_upload copies to the device and records in the context.
struct CompiledScene {
  std::vector<DNode> nodes;
  std::vector<unsigned char> nodes4;  // n_nodes4 x DNode4F, or DNode4C for a book-2 scene (!exts.empty())
  std::vector<DPrim> prims;
  std::vector<DExt> exts;
  std::vector<DMat> mats;
  std::vector<DTex> texs;             // an image texture's img.texels is null: texels + img_off[table] on the device
  std::vector<DPerlin> perlin;
  std::vector<uint8_t> texels;
  std::vector<size_t> img_off;
  // hop_kind 2: the ground-stack record followed by its guard bitmap (rt_layout.h DGround); else empty
  std::vector<uint32_t> ground;
  // hop_planes: the stack's plane record (rt_layout.h DPlanes); else empty
  std::vector<uint32_t> planes;
  // device primitive number -> object index (primitives are numbered in the reference tree's leaf order)
  std::vector<int32_t> prim_object;
  // flattened rotated spheres (flat_object): object index -> RotateY's cos, sin, for rt_scene_hit's u, v
  std::vector<std::pair<int32_t, std::pair<double, double>>> uv_fixups;
  LightList lights;
  // device primitive number -> index into the light list, or -1 (rt_render_nee: which light a path landed on)
  std::vector<int32_t> prim_light;
  rt_scene_stats stats{};
  uint64_t digest = 0;
  int32_t n_perlin = 0;
  bool has_perlin = false;            // some texture is RT_TEX_PERLIN
  ScenePlacement place;
};

// Validates `d` and compiles it for `builder` (RT_BVH_* with placement bits).  RT_OK, or RT_E_INVALID /
// RT_E_UNSUPPORTED with a message in *err (may be null).  Calls no getenv.
int compile_scene(const rt_scene_desc* d, int32_t builder, const SceneTuning& tune, CompiledScene* out, std::string* err);

int validate(const rt_scene_desc* d, std::string* err);

// 64-bit FNV-1a digest of a scene description and its BVH builder, field by field (no struct padding
// hashed): rt_scene_digest / the multi-GPU scene check.
struct Fnv1a {
  uint64_t h = 14695981039346656037ull;
  void bytes(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  }
  template <class T>
  void val(const T& v) { bytes(&v, sizeof v); }
};
uint64_t scene_digest(const rt_scene_desc* d, int32_t builder);

// rt_bvh_build_host / rt_scene_hit_ex share these with compile_scene
rt_scene_desc flat_scene(const rt_scene_desc* d, std::vector<rt_object>& store);
BuiltTree build_tree(const rt_scene_desc* d, int32_t builder, const SceneTuning& tune);
void box_to6(const Box& b, double* o);
void instance_sphere_uv(double cs, double sn, rt_hit& h);

}  // namespace rt
