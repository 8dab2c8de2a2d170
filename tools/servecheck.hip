// Bit-identity check, on the GPU, of the serve body written out for a y face (rt_device.h serve_y) against the general
// device functions it replaces in the HOP = 4 instances: hit_record<false, false> + unit_fast + shade_dielectric.
// Usage: servecheck [log2 cases]   (default 20)
// One thread per case, the families of tests/serve_y_check.c: random directions at lengths 2^-300 ..
// 2^300; d.x, d.z +-0; components so small that ud underflows or is subnormal; normal incidence; grazing rays; |d| at
// and beyond both ends of unit_fast's range; cos_theta a few ulps either side of total internal reflection; the
// uniform on and an ulp either side of the reflectance — over indices 1.0, 1.3, 1/1.3, 1.5, 1/1.5, faces 4 and 5, both
// sides.  Both forms start from the same (o, d, t, Rng, uniform): the new o, d and rng.draw / c2 / c3 must carry the
// same bits.  The lanes serve_y hands back (they run the general body in the kernels) are counted: this is where the
// fallback is certain to run on the device.  Prints the counts; exit code 1 if any case differs.
#include "../shirley-raytracing-rs_amd/csrc/rt/rt_device.h"
#include <cstdio>
#include <cstdlib>

using namespace rt;

__device__ __forceinline__ uint64_t mix(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
struct Gen {
  uint64_t s;
  __device__ uint64_t next() { return s = mix(s + 0x9E3779B97F4A7C15ull); }
  __device__ double unif() { return (double)(next() >> 11) * 0x1p-53; }
  __device__ double range(double a, double b) { return a + (b - a) * unif(); }
  __device__ double sgn() { return (next() & 1) ? 1.0 : -1.0; }
  __device__ double tiny() {
    switch (next() % 5) {
      case 0: return 0x1p-1074 * (double)(1 + next() % 7);
      case 1: return ldexp(range(1.0, 2.0), -1074 + (int)(next() % 60));
      case 2: return ldexp(range(1.0, 2.0), -1022 - (int)(next() % 4));
      case 3: return ldexp(range(1.0, 2.0), -1022 + (int)(next() % 4));
      default: return ldexp(range(1.0, 2.0), -301 + (int)(next() % 3));  // either side of 2^-300
    }
  }
};
__device__ __forceinline__ double ulps(double x, int k) {
  for (; k > 0; --k) x = nextafter(x, __builtin_inf());
  for (; k < 0; ++k) x = nextafter(x, -__builtin_inf());
  return x;
}
__device__ __forceinline__ bool same(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

// counts: 0 differing cases, 1 served by serve_y, 2 handed back, 3 totally reflected, 4 reflected by the draw, 5 refracted
__global__ void check(uint64_t n, unsigned long long* cnt) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  Gen g{mix(i * 0x2545F4914F6CDD1Dull + 1)};
  const double irs[5] = {1.0, 1.3, 1.0 / 1.3, 1.5, 1.0 / 1.5};
  const double ir = irs[i % 5];
  const int fam = (int)((i / 5) % 8), face = 4 + (int)((i / 40) & 1);
  const bool down = ((i / 80) & 1) != 0;
  const double sy = down ? -1.0 : 1.0;
  DMat m{};
  m.kind = RT_MAT_DIELECTRIC;
  m.param = ir;
  m.inv_param = 1.0 / ir;
  for (int k = 0; k < 2; ++k) {  // scene_compile.cpp: Schlick's r0^2 for the front / back face ratio
    const double rk = k ? m.param : m.inv_param, r0 = (1.0 - rk) / (1.0 + rk);
    m.albedo[k] = r0 * r0;
  }
  const double ratio = down ? m.inv_param : m.param;
  v3 d = V(g.range(-1.0, 1.0), sy * g.range(0.05, 1.0), g.range(-1.0, 1.0));
  double u = g.unif();
  switch (fam) {
    case 0:
    case 7: d = scale(d, ldexp(1.0, (int)(g.next() % 601) - 300)); break;
    case 1: {
      const int w = 1 + (int)(g.next() % 3);
      if (w & 1) d.x = 0.0 * g.sgn();
      if (w & 2) d.z = 0.0 * g.sgn();
      if (g.next() & 1) d = scale(d, ldexp(1.0, (int)(g.next() % 401) - 200));
      break;
    }
    case 2: {
      const int w = 1 + (int)(g.next() % 3);
      if (w & 1) d.x = g.tiny() * g.sgn();
      if (w & 2) d.z = g.tiny() * g.sgn();
      if (g.next() % 4 == 0) d.y = sy * ldexp(g.range(1.0, 2.0), (int)(g.next() % 40));
      break;
    }
    case 3: {
      const int w = (int)(g.next() % 4);
      d.y = sy * ((g.next() & 1) ? ldexp(1.0, (int)(g.next() % 41) - 20) : g.range(0.5, 4.0));
      d.x = w == 0 ? 0.0 * g.sgn() : w == 1 ? g.tiny() * g.sgn() : d.y * ldexp(g.range(-1.0, 1.0), -27 - (int)(g.next() % 30));
      d.z = w == 0 ? 0.0 * g.sgn() : w == 2 ? g.tiny() * g.sgn() : d.y * ldexp(g.range(-1.0, 1.0), -27 - (int)(g.next() % 30));
      break;
    }
    case 4:
      d.y = sy * exp(g.range(log(1e-7), log(1e-2)));
      if (g.next() & 1) d = scale(d, ldexp(1.0, (int)(g.next() % 201) - 100));
      break;
    case 5: {
      const int e = 290 + (int)(g.next() % 31);
      d = scale(d, ldexp(1.0, (g.next() & 1) ? e : -e));
      break;
    }
    case 6: {
      const double phi = g.range(0.0, 6.283185307179586);
      if (ratio > 1.0) {
        const double c = ulps(sqrt(1.0 - 1.0 / (ratio * ratio)), (int)(g.next() % 9) - 4), s = sqrt(1.0 - c * c);
        d = V(s * cos(phi), sy * c, s * sin(phi));
        if (g.next() & 1) d = scale(d, g.range(0.5, 2.0));
      } else {
        const double c = g.unif(), s = sqrt(1.0 - c * c);
        d = V(s * cos(phi), sy * fmax(c, 1e-9), s * sin(phi));
      }
      break;
    }
  }
  DPrim pr{};
  pr.kind = kPrimBox;
  pr.material = 0;
  pr.p[0] = -4.0, pr.p[1] = -0.0078125, pr.p[2] = -4.0, pr.p[3] = 4.0, pr.p[4] = 0.0, pr.p[5] = 4.0;
  const double yf = face == 4 ? pr.p[4] : pr.p[1];
  v3 o = V(g.range(-4.0, 4.0), yf - sy * g.range(0.001, 0.5), g.range(-4.0, 4.0));
  if (g.next() % 8 == 0) o.x = 0.0 * g.sgn();
  const double t = (yf - o.y) / d.y;
  if (fam == 7) {  // the uniform on, and an ulp either side of, the reflectance the general body compares it with
    const v3 ud = unit_fast(d);
    u = ulps(reflectance_r0sq(fmin_one(fabs(ud.y)), down ? m.albedo[0] : m.albedo[1]), (int)(g.next() % 3) - 1);
  }
  const uint64_t cache = g.next();
  const v3 ru = V(u, u64_as_double(cache), 0.0);
  const Rng rng0{(uint32_t)(i & 0xffffu), (uint32_t)(i >> 16), (uint32_t)(g.next() % 100), (uint32_t)g.next(), (uint32_t)g.next()};
  // the general body
  DScene S{};
  Rng ra = rng0;
  v3 oa = o, da = d;
  Hit hh;
  hit_record<false, false>(S, pr, face, oa, da, t, ra, 0ull, hh);
  shade_dielectric(m, ru, unit_fast(da), ra, oa, da, hh);
  // serve_y; a lane it hands back runs the general body in the kernels, so its outputs are those above
  Rng rb = rng0;
  v3 ob = o, db = d;
  const bool by_y = serve_y(m, ru, rb, ob, db, t);
  if (!by_y) {
    if (!(same(ob.x, o.x) && same(ob.y, o.y) && same(ob.z, o.z) && same(db.x, d.x) && same(db.y, d.y) && same(db.z, d.z) &&
          rb.draw == rng0.draw && rb.c2 == rng0.c2 && rb.c3 == rng0.c3))
      atomicAdd(&cnt[0], 1ull);  // (handed back with something changed)
    atomicAdd(&cnt[2], 1ull);
    return;
  }
  atomicAdd(&cnt[1], 1ull);
  if (!(same(oa.x, ob.x) && same(oa.y, ob.y) && same(oa.z, ob.z) && same(da.x, db.x) && same(da.y, db.y) && same(da.z, db.z) &&
        ra.draw == rb.draw && ra.c2 == rb.c2 && ra.c3 == rb.c3))
    atomicAdd(&cnt[0], 1ull);
  const bool drew = ra.draw != rng0.draw, reflected = same(da.y, -unit_fast(d).y) && same(da.x, unit_fast(d).x);
  atomicAdd(&cnt[!drew ? 3 : reflected ? 4 : 5], 1ull);
}

int main(int argc, char** argv) {
  const int lg = argc > 1 ? atoi(argv[1]) : 20;
  if (lg < 8 || lg > 28) return 2;
  unsigned long long* cnt;
  if (hipMalloc(&cnt, 48) != hipSuccess) return 2;
  (void)hipMemset(cnt, 0, 48);
  const uint64_t n = 1ull << lg;
  hipLaunchKernelGGL(check, dim3((unsigned)(n / 256)), dim3(256), 0, 0, n, cnt);
  unsigned long long h[6];
  if (hipMemcpy(h, cnt, 48, hipMemcpyDeviceToHost) != hipSuccess) return 2;
  printf("servecheck: %llu cases, %llu differ, %llu by serve_y, %llu handed back, %llu totally reflected, %llu reflected, "
         "%llu refracted\n", (unsigned long long)n, h[0], h[1], h[2], h[3], h[4], h[5]);
  return h[0] ? 1 : 0;
}
