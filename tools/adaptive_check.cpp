// adaptive_check — prints the rules of csrc/rt/adaptive.h (validation, step schedule, list compaction,
// tile error) for the query on the command line, so tests/test_adaptive_plan.py checks them on the CPU.
//   adaptive_check validate <samples> <sample_chunk> <sample_begin> <sample_count> <tile_world> <min> <step> <threshold> <floor>
//       -> "ok <batch>" or "invalid <message>"
//   adaptive_check schedule <samples> <sample_chunk> <min> <step>       -> one "<begin> <end>" line per step
//   adaptive_check compact <threshold> <tile>:<error> ...               -> the tiles that go on, one line
//   adaptive_check error <n> <b> <noise_floor> <m1>:<m2> ...            -> v_p per pixel, then E, M and e (%.17g)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../shirley-raytracing-rs_amd/csrc/rt/adaptive.h"

namespace {
rt_render_params render_params(int samples, int chunk) {
  rt_render_params p{};
  p.samples = samples;
  p.max_depth = 50;
  p.sample_chunk = chunk;
  p.tile_world = 1;
  return p;
}
}  // namespace

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!std::strcmp(mode, "validate") && argc == 11) {
    rt_render_params p = render_params(std::atoi(argv[2]), std::atoi(argv[3]));
    p.sample_begin = std::atoi(argv[4]);
    p.sample_count = std::atoi(argv[5]);
    p.tile_world = std::atoi(argv[6]);
    rt_adaptive_params a{std::atoi(argv[7]), std::atoi(argv[8]), std::strtod(argv[9], nullptr), std::strtod(argv[10], nullptr)};
    rt::AdaptivePlan plan;
    const char* why = rt::adaptive_validate(&p, &a, &plan);
    if (why) std::printf("invalid %s\n", why);
    else std::printf("ok %d\n", plan.batch);
    return 0;
  }
  if (!std::strcmp(mode, "schedule") && argc == 6) {
    const rt_render_params p = render_params(std::atoi(argv[2]), std::atoi(argv[3]));
    const rt_adaptive_params a{std::atoi(argv[4]), std::atoi(argv[5]), 0.0, 0.0};
    rt::AdaptivePlan plan;
    if (const char* why = rt::adaptive_validate(&p, &a, &plan)) {
      std::printf("invalid %s\n", why);
      return 0;
    }
    for (int k = 0; k < rt::adaptive_n_steps(plan); ++k) {
      int b = 0, e = 0;
      rt::adaptive_step_range(plan, k, &b, &e);
      std::printf("%d %d\n", b, e);
    }
    return 0;
  }
  if (!std::strcmp(mode, "compact") && argc >= 3) {
    const double threshold = std::strtod(argv[2], nullptr);
    std::vector<uint32_t> list;
    std::vector<double> err;
    for (int i = 3; i < argc; ++i) {
      char* colon = nullptr;
      list.push_back((uint32_t)std::strtoul(argv[i], &colon, 10));
      err.push_back(std::strtod(colon + 1, nullptr));
    }
    std::vector<uint32_t> next(list.size() + 1);
    const size_t m = rt::adaptive_compact(list.data(), err.data(), list.size(), threshold, next.data());
    for (size_t i = 0; i < m; ++i) std::printf("%u ", next[i]);
    std::printf("\n");
    return 0;
  }
  if (!std::strcmp(mode, "error") && argc >= 6) {
    const long long n = std::atoll(argv[2]);
    const int b = std::atoi(argv[3]);
    const double floor = std::strtod(argv[4], nullptr);
    double E = 0.0, M = 0.0;
    int K = 0;
    for (int i = 5; i < argc; ++i, ++K) {
      char* colon = nullptr;
      const double m1 = std::strtod(argv[i], &colon), m2 = std::strtod(colon + 1, nullptr);
      const double v = rt::pixel_variance(m1, m2, n);
      std::printf("%.17g\n", v);
      E += v;
      M += m1;
    }
    const double e = rt::tile_error(E, M, K, n, b, floor);
    std::printf("%.17g %.17g %.17g\n", E, M, e);
    std::printf("%s\n", rt::tile_continues(e, 0.5) ? "continues" : "stops");  // (the stop rule at threshold 0.5)
    return 0;
  }
  std::fprintf(stderr, "usage: %s validate|schedule|compact|error ... (see the file's head)\n", argv[0]);
  return 2;
}
