// ground_stack — prints rt::compile_scene's choice of hop pass (ScenePlacement.hop_kind, rt_scene_stats.hop_kind)
// and the scene's ground-stack record (rt_layout.h DGround), and checks the record's guard bitmap by brute
// force, so tests/test_ground_hop.py checks the rule on the CPU.  Links scene_compile.cpp, bvh_build.cpp and
// the host layer; no HIP.
//   ground_stack <case>[/KEY=VALUE[,KEY=VALUE...]] ...
//     case       a builtin of sh_scene_builtin (random, cornell, ...) or @<file>: a scene saved as JSON
//     KEY=VALUE  the upload-time tuning variable SHIRLEY_<KEY>, set for this case only
// prints one JSON line per case; `hop_down`: the launches take the down pass's instances (ScenePlacement.hop_down);
// `hop_planes`, `hop_instance`: ... those of a plane stack (ScenePlacement.hop_planes), with its record (rt_layout.h
// DPlanes): `planes` the sorted y values as hex floats, `plane_info` their packed words, `core` the shrunk core and `tol`.
// Guard check: every cell against the distance from its rectangle to the nearest contact point over all spheres
// (`cells_wrong`), and 256 points on and inside the guard circle of every guarded sphere, which must all fall in
// marked cells (`points_free`).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/shirley_host.h"
#include "../shirley-raytracing-rs_amd/csrc/rt/scene_compile.h"

int main(int argc, char** argv) {
  const uint64_t seed = 0x5EED;
  for (int a = 1; a < argc; ++a) {
    std::string name = argv[a], keys_arg;
    const size_t slash = name.rfind('/');
    if (slash != std::string::npos && name.find('=', slash) != std::string::npos) {
      keys_arg = name.substr(slash + 1);
      name = name.substr(0, slash);
    }
    sh_scene* s = nullptr;
    int rc;
    if (name[0] == '@') {
      std::ifstream in(name.substr(1));
      std::stringstream ss;
      ss << in.rdbuf();
      rc = sh_scene_from_json(ss.str().c_str(), &s);
    } else {
      rc = sh_scene_builtin(name.c_str(), seed, &s);
    }
    sh_desc* desc = nullptr;
    if (rc != 0 || !s || sh_scene_finalize(s, seed, &desc) != 0) {
      std::fprintf(stderr, "ground_stack: %s: %s\n", argv[a], sh_last_error());
      return 2;
    }
    std::vector<std::string> keys;
    std::stringstream ks(keys_arg);
    for (std::string kv; std::getline(ks, kv, ',');) {
      const size_t eq = kv.find('=');
      keys.push_back("SHIRLEY_" + kv.substr(0, eq));
      setenv(keys.back().c_str(), kv.substr(eq + 1).c_str(), 1);
    }
    const rt::SceneTuning tune = rt::tuning_from_env();
    for (const std::string& k : keys) unsetenv(k.c_str());

    rt::CompiledScene cs;
    std::string err;
    const int st = rt::compile_scene(sh_desc_view(desc), RT_BVH_SAH, tune, &cs, &err);
    std::printf("{\"case\": \"%s\", \"status\": %d, \"hop_pass\": %d, \"hop_kind\": %d, \"stats_hop_kind\": %d, "
                "\"hop_down\": %d, \"hop_planes\": %d, \"hop_instance\": %d", argv[a], st, cs.place.hop_pass ? 1 : 0,
                cs.place.hop_kind, (int)cs.stats.hop_kind, cs.place.hop_down ? 1 : 0, cs.place.hop_planes ? 1 : 0,
                rt::hop_instance(cs.place));
    if (st == 0 && cs.exts.empty()) {
      // the geometry kinds of the leaf children of the first 4-wide node a traversal visits (0 a sphere)
      rt::DNode4F nd;
      std::memcpy(&nd, cs.nodes4.data() + (size_t)cs.place.root4 * sizeof nd, sizeof nd);
      std::printf(", \"root_leaf_kinds\": [");
      bool first = true;
      for (int k = 0; k < 4; ++k)
        if (nd.child[k] < 0) {
          std::printf("%s%d", first ? "" : ", ", (int)cs.prims[(~nd.child[k]) & rt::kLeafPrimMask].kind);
          first = false;
        }
      std::printf("]");
    }
    if (st == 0 && cs.place.hop_planes) {
      rt::DPlanes pl;
      std::memcpy(&pl, cs.planes.data(), sizeof pl);
      std::printf(", \"planes\": [");
      for (int k = 0; k < pl.n; ++k) std::printf("%s\"%a\"", k ? ", " : "", pl.y[k]);
      std::printf("], \"plane_info\": [");
      for (int k = 0; k < pl.n; ++k) std::printf("%s%d", k ? ", " : "", pl.info[k]);
      std::printf("], \"core\": [\"%a\", \"%a\", \"%a\", \"%a\"], \"tol\": \"%a\"", pl.x0, pl.x1, pl.z0, pl.z1, pl.tol);
      // (plane_first's own core and origin-height bound)
      std::printf(", \"core_first\": [\"%a\", \"%a\", \"%a\", \"%a\"], \"y_max\": \"%a\", \"outer\": [\"%a\", \"%a\", \"%a\", \"%a\"]", pl.fx0,
                  pl.fx1, pl.fz0, pl.fz1, pl.y_max, pl.ox0, pl.ox1, pl.oz0, pl.oz1);
    }
    if (st == 0 && cs.place.hop_kind == 2) {
      rt::DGround g;
      std::memcpy(&g, cs.ground.data(), sizeof g);
      const uint32_t* bits = cs.ground.data() + sizeof g / 4;
      auto marked = [&](int i, int k) {
        const size_t c = (size_t)k * (size_t)g.nx + (size_t)i;
        return (bits[c >> 5] >> (c & 31)) & 1u;
      };
      std::vector<const rt::DPrim*> guarded;
      for (const rt::DPrim& q : cs.prims)
        if (q.kind == rt::kPrimSphere && !(q.p[3] <= 0.0 && q.p[1] - q.p[3] >= q.p[1] + q.p[3]) &&  // (never hit)
            (q.p[1] - q.p[3]) - g.y_top < rt::kGroundGuard / 2)
          guarded.push_back(&q);
      long long n_marked = 0, cells_wrong = 0, points_free = 0;
      const double rad = rt::kGroundGuard * (1.0 + 0x1p-20);
      for (int k = 0; k < g.nz; ++k)
        for (int i = 0; i < g.nx; ++i) {
          const double x_lo = g.x0 + i * rt::kGroundCell, z_lo = g.z0 + k * rt::kGroundCell;
          double best = INFINITY;
          for (const rt::DPrim* q : guarded) {
            const double ax = x_lo - q->p[0], bx = q->p[0] - (x_lo + rt::kGroundCell);
            const double az = z_lo - q->p[2], bz = q->p[2] - (z_lo + rt::kGroundCell);
            const double dx = ax > 0.0 ? ax : (bx > 0.0 ? bx : 0.0), dz = az > 0.0 ? az : (bz > 0.0 ? bz : 0.0);
            const double d2 = dx * dx + dz * dz;
            if (d2 < best) best = d2;
          }
          const bool m = marked(i, k);
          n_marked += m;
          cells_wrong += m != (best <= rad * rad);
        }
      for (const rt::DPrim* q : guarded)
        for (int j = 0; j < 256; ++j) {
          const double ang = 6.283185307179586 * (j % 64) / 64.0, rho = rt::kGroundGuard * (1.0 - (j / 64) / 4.0);
          const int i = rt::ground_cell(q->p[0] + rho * std::cos(ang), g.x0, g.nx);
          const int k = rt::ground_cell(q->p[2] + rho * std::sin(ang), g.z0, g.nz);
          points_free += !(i >= 0 && k >= 0 && marked(i, k));
        }
      std::printf(", \"n\": %d, \"n_box\": %d, \"y_lo\": %.17g, \"y_hi\": %.17g, \"y_top\": %.17g, \"dy_min\": %.17g, "
                  "\"ratio2\": %.17g, \"nx\": %d, \"nz\": %d, \"guard_bytes\": %zu, \"guarded_spheres\": %zu, "
                  "\"cells_marked\": %lld, \"cells_wrong\": %lld, \"points_free\": %lld",
                  g.n, g.n_box, g.y_lo, g.y_hi, g.y_top, g.dy_min, g.ratio2, g.nx, g.nz,
                  (cs.ground.size() - sizeof g / 4) * 4, guarded.size(), n_marked, cells_wrong, points_free);
    }
    std::printf("}\n");
    sh_desc_free(desc);
    sh_scene_free(s);
  }
  return 0;
}
