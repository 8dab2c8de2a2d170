// denoise_check — csrc/rt/denoise.h on the CPU as a stand-alone program (tests/test_denoise.py builds it
// plainly and with AddressSanitizer + UBSan): the argument rules and the whole filter (denoise_host, what
// rt_denoise runs) on a frame read from a file.
//
//   denoise_check validate W H samples feature_samples has_counts iterations normal_power_log2
//                          sigma_z sigma_a sigma_c albedo_floor        -> "ok" | "invalid <why>"
//   denoise_check filter IN OUT
//     IN : int32 W, H, samples, feature_samples, has_counts, has_variance, iterations, normal_power_log2;
//          f64 sigma_z, sigma_a, sigma_c, albedo_floor; f64 accum[H][W][3], albedo[H][W][3], normal[H][W][3],
//          depth[H][W]; int32 counts[H][W] if has_counts; f64 variance[H][W] if has_variance
//     OUT: f64 out[H][W][3]
//   denoise_check variance batch m1:m2:count ...                       -> one value per pixel
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../shirley-raytracing-rs_amd/csrc/rt/denoise.h"

using namespace rt;

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "validate" && argc == 13) {
    static const double one[3] = {1.0, 1.0, 1.0};
    rt_denoise_inputs in{};
    rt_denoise_params p{};
    in.width = atoi(argv[2]);
    in.height = atoi(argv[3]);
    in.samples = atoi(argv[4]);
    in.feature_samples = atoi(argv[5]);
    static const int32_t cnt[1] = {1};
    in.counts = atoi(argv[6]) ? cnt : nullptr;
    in.accum = in.albedo = in.normal = in.depth = one;
    p.iterations = atoi(argv[7]);
    p.normal_power_log2 = atoi(argv[8]);
    p.sigma_z = atof(argv[9]);
    p.sigma_a = atof(argv[10]);
    p.sigma_c = atof(argv[11]);
    p.albedo_floor = atof(argv[12]);
    const char* why = denoise_validate(&in, &p);
    printf("%s%s\n", why ? "invalid " : "ok", why ? why : "");
    return 0;
  }
  if (mode == "variance" && argc >= 3) {
    const int batch = atoi(argv[2]);
    for (int i = 3; i < argc; ++i) {
      double m1, m2;
      int count;
      if (sscanf(argv[i], "%lf:%lf:%d", &m1, &m2, &count) != 3) return 2;
      printf("%.17g\n", dn_moments_variance(m1, m2, count, batch));
    }
    return 0;
  }
  if (mode == "filter" && argc == 4) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 3;
    int32_t hd[8];
    double sg[4];
    if (!read_all(f, hd, sizeof hd) || !read_all(f, sg, sizeof sg)) return 3;
    const int W = hd[0], H = hd[1];
    if (W < 1 || H < 1 || W > 4096 || H > 4096) return 3;
    const size_t n = (size_t)W * H;
    std::vector<double> accum(n * 3), albedo(n * 3), normal(n * 3), depth(n), var(hd[5] ? n : 0);
    std::vector<int32_t> counts(hd[4] ? n : 0);
    if (!read_all(f, accum.data(), n * 24) || !read_all(f, albedo.data(), n * 24) ||
        !read_all(f, normal.data(), n * 24) || !read_all(f, depth.data(), n * 8) ||
        !read_all(f, counts.data(), counts.size() * 4) || !read_all(f, var.data(), var.size() * 8))
      return 3;
    fclose(f);
    rt_denoise_inputs in{};
    in.width = W;
    in.height = H;
    in.samples = hd[2];
    in.feature_samples = hd[3];
    in.accum = accum.data();
    in.albedo = albedo.data();
    in.normal = normal.data();
    in.depth = depth.data();
    in.counts = hd[4] ? counts.data() : nullptr;
    in.variance = hd[5] ? var.data() : nullptr;
    rt_denoise_params p{};
    p.iterations = hd[6];
    p.normal_power_log2 = hd[7];
    p.sigma_z = sg[0];
    p.sigma_a = sg[1];
    p.sigma_c = sg[2];
    p.albedo_floor = sg[3];
    std::vector<double> out(n * 3);
    if (const char* why = denoise_host(&in, &p, out.data())) {
      printf("invalid %s\n", why);
      return 0;
    }
    FILE* g = fopen(argv[3], "wb");
    if (!g || fwrite(out.data(), 8, out.size(), g) != out.size()) return 3;
    fclose(g);
    printf("ok\n");
    return 0;
  }
  return 2;
}
