// hop_flag — prints rt::compile_scene's hop-pass decision (ScenePlacement.hop_pass, rt_scene_stats.hop_pass)
// for a few hand-built scenes, so tests/test_hop_flag.py checks the rule on the CPU.  Links scene_compile.cpp
// and bvh_build.cpp; no HIP, no host layer.
//   hop_flag <case> ...   case: box | sphere | book2 | box_nohop | box_global
// prints one JSON line per case.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../shirley-raytracing-rs_amd/csrc/rt/scene_compile.h"

namespace {

rt_object object(int32_t geometry, int32_t material, double p0, double p1, double p2, double p3, double p4, double p5) {
  rt_object o;
  std::memset(&o, 0, sizeof o);
  o.geometry = geometry;
  o.material = material;
  const double p[6] = {p0, p1, p2, p3, p4, p5};
  for (int k = 0; k < 6; ++k) o.p[k] = p[k];
  return o;
}

}  // namespace

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    const std::string name = argv[a];
    // materials: 0 = dielectric(1.5), 1 = metal
    rt_material mats[2];
    std::memset(mats, 0, sizeof mats);
    mats[0].kind = RT_MAT_DIELECTRIC;
    mats[0].param = 1.5;
    mats[1].kind = RT_MAT_METAL;
    mats[1].albedo[0] = mats[1].albedo[1] = mats[1].albedo[2] = 0.5;
    std::vector<rt_object> objs;
    objs.push_back(object(RT_GEOM_SPHERE, 1, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0));  // a metal sphere in every scene
    if (name == "sphere") {
      objs.push_back(object(RT_GEOM_SPHERE, 0, 3.0, 1.0, 0.0, 1.0, 0.0, 0.0));
    } else {
      objs.push_back(object(RT_GEOM_RECT_BOX, 0, -10.0, -0.01, -10.0, 10.0, 0.0, 10.0));
      if (name == "book2") {  // a moving sphere: an extended object
        rt_object m = object(RT_GEOM_MOVING_SPHERE, 1, 3.0, 1.0, 0.0, 0.5, 0.0, 0.0);
        m.q[0] = 3.0, m.q[1] = 1.5, m.q[2] = 0.0, m.q[3] = 0.0, m.q[4] = 1.0;
        objs.push_back(m);
      }
    }
    rt_scene_desc d;
    std::memset(&d, 0, sizeof d);
    d.sky = RT_SKY_ABOVE;
    d.n_objects = (int32_t)objs.size();
    d.objects = objs.data();
    d.n_materials = 2;
    d.materials = mats;
    rt::SceneTuning tune;
    tune.no_hop = name == "box_nohop";
    const int32_t builder = RT_BVH_SAH | (name == "box_global" ? RT_BVH_NODES_GLOBAL : 0);
    rt::CompiledScene cs;
    std::string err;
    const int st = rt::compile_scene(&d, builder, tune, &cs, &err);
    std::printf("{\"case\": \"%s\", \"status\": %d, \"hop_pass\": %d, \"stats_hop_pass\": %d, \"n_exts\": %zu, "
                "\"n_lds_prims\": %d, \"mk_threads\": %d}\n",
                name.c_str(), st, cs.place.hop_pass ? 1 : 0, (int)cs.stats.hop_pass, cs.exts.size(),
                cs.place.n_lds_prims, cs.place.mk_threads);
  }
  return 0;
}
