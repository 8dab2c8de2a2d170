// scene_plan — prints rt::compile_scene (csrc/rt/scene_compile.h: the compiled tables and the placement
// plan of a scene) for the cases given on the command line, so tests/test_scene_plan.py checks scene
// compilation on the CPU.  Links scene_compile.cpp, bvh_build.cpp and the host layer; no HIP.
//   scene_plan <scene>/<seed>/<builder>/<placement>[/KEY=VALUE[,KEY=VALUE...]] ...
//     scene      a builtin of sh_scene_builtin (random, final:4:30, spheres:11, ...), or `empty` (no object),
//                or `one` (one sphere)
//     builder    reference | sah
//     placement  default | global | half_lds | lds
//     KEY=VALUE  the upload-time tuning variable SHIRLEY_<KEY>, set for this case only
// prints one JSON line per case: the digest, every ScenePlacement field, the tree's sizes and an FNV-1a of
// the bytes of each compiled table (an image texture's device pointer is null here).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/shirley_host.h"
#include "../shirley-raytracing-rs_amd/csrc/rt/scene_compile.h"

namespace {

std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out(1);
  for (char ch : s)
    if (ch == sep) out.emplace_back();
    else out.back() += ch;
  return out;
}

template <class V>
uint64_t table_hash(const V& v) {
  rt::Fnv1a f;
  f.bytes(v.data(), v.size() * sizeof v[0]);
  return f.h;
}

int usage(const char* what) {
  std::fprintf(stderr, "scene_plan: %s\nusage: scene_plan <scene>/<seed>/<reference|sah>/<default|global|half_lds|lds>"
                       "[/KEY=VALUE,...] ...\n", what);
  return 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return usage("no case");
  for (int a = 1; a < argc; ++a) {
    const std::vector<std::string> f = split(argv[a], '/');
    if (f.size() < 4 || f.size() > 5) return usage(argv[a]);
    const uint64_t seed = std::strtoull(f[1].c_str(), nullptr, 0);
    int32_t builder;
    if (f[2] == "reference") builder = RT_BVH_REFERENCE;
    else if (f[2] == "sah") builder = RT_BVH_SAH;
    else return usage(argv[a]);
    if (f[3] == "global") builder |= RT_BVH_NODES_GLOBAL;
    else if (f[3] == "half_lds") builder |= RT_BVH_NODES_HALF_LDS;
    else if (f[3] == "lds") builder |= RT_BVH_NODES_LDS;
    else if (f[3] != "default") return usage(argv[a]);

    sh_scene* s = nullptr;
    if (f[0] == "empty" || f[0] == "one") {
      s = sh_scene_new();
      if (f[0] == "one" &&
          sh_scene_add_json(s, "{\"geometry\":{\"Sphere\":{\"center\":{\"vec\":[0.5,1.0,-2.0]},\"radius\":1.25}},"
                               "\"material\":{\"Metal\":{\"albedo\":{\"vec\":[0.8,0.6,0.2]},\"fuzz\":0.25}}}") != 0)
        return usage(sh_last_error());
    } else if (sh_scene_builtin(f[0].c_str(), seed, &s) != 0) {
      return usage(sh_last_error());
    }
    sh_desc* desc = nullptr;
    if (!s || sh_scene_finalize(s, seed, &desc) != 0) return usage(sh_last_error());

    std::vector<std::string> keys;
    if (f.size() == 5)
      for (const std::string& kv : split(f[4], ',')) {
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) return usage(argv[a]);
        keys.push_back("SHIRLEY_" + kv.substr(0, eq));
        setenv(keys.back().c_str(), kv.substr(eq + 1).c_str(), 1);
      }
    const rt::SceneTuning tune = rt::tuning_from_env();
    for (const std::string& k : keys) unsetenv(k.c_str());

    rt::CompiledScene cs;
    std::string err;
    const int st = rt::compile_scene(sh_desc_view(desc), builder, tune, &cs, &err);
    if (st) {
      std::printf("{\"case\": \"%s\", \"status\": %d, \"error\": \"%s\"}\n", argv[a], st, err.c_str());
    } else {
      const rt::ScenePlacement& P = cs.place;
      std::printf("{\"case\": \"%s\", \"status\": 0, \"digest\": \"%016" PRIx64 "\", ", argv[a], cs.digest);
      std::printf("\"wide\": %d, \"mk_threads\": %d, \"collapse_dp\": %d, \"n_lds_nodes\": %d, \"n_lds_nodes4\": %d, "
                  "\"n_lds_prims\": %d, \"n_lds_perlin\": %d, \"n_lds_mats\": %d, \"n_lds_texs\": %d, ",
                  P.wide ? 1 : 0, P.mk_threads, P.collapse_dp ? 1 : 0, P.n_lds_nodes, P.n_lds_nodes4, P.n_lds_prims,
                  P.n_lds_perlin, P.n_lds_mats, P.n_lds_texs);
      std::printf("\"stack_depth\": %d, \"stack_depth4\": %d, \"root4\": %d, \"stack_bytes\": %lld, \"key_mask\": %u, "
                  "\"origin_limit\": %.9g, \"wf_n_lds_nodes\": %d, \"wf_extend4\": %d, \"split_nt\": %d, "
                  "\"split_refill\": %d, ",
                  P.stack_depth, P.stack_depth4, P.root4, P.stack_bytes, P.key_mask, (double)P.origin_limit,
                  P.wf_n_lds_nodes, P.wf_extend4 ? 1 : 0, P.split_nt, P.split_refill);
      std::printf("\"n_objects\": %d, \"n_nodes\": %d, \"n_nodes4\": %d, \"n_leaves\": %d, \"depth\": %d, "
                  "\"device_bytes\": %lld, \"n_exts\": %zu, \"n_uv_fixups\": %zu, \"n_perlin\": %d, \"has_perlin\": %d, ",
                  cs.stats.n_objects, cs.stats.n_nodes, cs.stats.n_nodes4, cs.stats.n_leaves, cs.stats.depth,
                  (long long)cs.stats.device_bytes, cs.exts.size(), cs.uv_fixups.size(), cs.n_perlin,
                  cs.has_perlin ? 1 : 0);
      std::printf("\"fnv\": {\"nodes\": \"%016" PRIx64 "\", \"nodes4\": \"%016" PRIx64 "\", \"prims\": \"%016" PRIx64
                  "\", \"exts\": \"%016" PRIx64 "\", \"mats\": \"%016" PRIx64 "\", \"texs\": \"%016" PRIx64
                  "\", \"perlin\": \"%016" PRIx64 "\", \"texels\": \"%016" PRIx64 "\", \"prim_object\": \"%016" PRIx64
                  "\"}}\n",
                  table_hash(cs.nodes), table_hash(cs.nodes4), table_hash(cs.prims), table_hash(cs.exts),
                  table_hash(cs.mats), table_hash(cs.texs), table_hash(cs.perlin), table_hash(cs.texels),
                  table_hash(cs.prim_object));
    }
    sh_desc_free(desc);
    sh_scene_free(s);
  }
  return 0;
}
