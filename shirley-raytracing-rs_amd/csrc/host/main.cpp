// main.cpp — ray-cli: the reference's CLI (src/main.rs, src/argparse.rs) on the C++ host, with
// render_scene (main.rs:65-130) calling the MI355X render ABI instead of the rayon scanline loop.
//
//   ray-cli [-v...] render <random|saved|demo|perlin|earth|box-light|cornell|spheres|final> [options]
//   ray-cli test
//
// Reference flags (argparse.rs:106-167): -o/--output out.png, -s/--samples 100, -m/--max-reflect 50,
// --single-threaded (accepted; the GPU path has no CPU thread count), -w/--width 640, --camera-fov 20,
// --camera-focal-length 1.0, --camera-aperture 0.001, --camera-aspect-ratio std3x2;
// random: --night, --scene-output FILE; saved: <scene_input>.
// Added: --seed N (the reference is unseeded), --device N, --bvh reference|sah, --sample-chunk N,
// --dump-accum FILE (raw f64 [H][W][3] sums, row 0 = bottom), --side-len N (spheres),
// --gpus N (devices [device, device + N): the frame's tiles sharded over N GPUs with an RCCL gather,
// rt_render_multi — the counterpart of the reference's whole-machine rayon loop, main.rs:117-125),
// --partition tiles|samples (how --gpus splits the frame, RT_PARTITION_*; default: the library's),
// --progressive K (the frame's samples in K consecutive ranges, rt_render_params.sample_begin / count;
// after each range the running sums go to --dump-accum FILE + FILE.json and the PNG shows the samples so
// far: a checkpoint), --resume FILE (continue from such a checkpoint: its sums cover samples [0, N)),
// --adaptive T (adaptive sampling, rt_render_adaptive: -s is the per-pixel maximum, an 8x8 tile stops when
// its relative error is <= T; --min-samples N and --adaptive-step N, multiples of --sample-chunk (0 = 4),
// --noise-floor F; the picture divides every pixel by its own sample count; one GPU, no checkpoints),
// --ao RADIUS (`inf` accepted) [--ao-chain K]: the ambient-occlusion pass (rt_render_ao) over the frame's
// samples in place of the colour render, written as a grey picture through the tonemap; one GPU, no
// checkpoints, no --adaptive / --denoise, no book-2 objects.
// --direct [--direct-chain K]: the direct-lighting pass (rt_render_direct) in place of the colour render — the
// feature vertex's emission plus the one-light-sample estimate from the scene's light list — through the
// tonemap; the same restrictions as --ao, and not together with it.
// --nee [--nee-mis 0|1]: the light-sampling path integrator (rt_render_nee; --nee-mis 1, the default, weights
// light sample and scatter by the balance heuristic) in place of the colour render, with the usual -s / -m;
// the same restrictions as --direct, and not together with it.
// --nee-adaptive T (with --nee): the adaptive light-sampling render (rt_render_nee_adaptive) — --adaptive's rule
// with --min-samples, --adaptive-step, --noise-floor and --sample-chunk, applied inside the one launch; the
// picture divides every pixel by its own sample count; --nee's restrictions.
// --light-grid N (with --nee or --direct): the spatially weighted light pick (rt_scene_light_pick) with N cells,
// 1 ... 64, along the light grid's longest axis; 0, the default, is the uniform pick.
// --light-visibility K (with --light-grid N >= 1): K shadow rays per cell and light weight the grid's rows
// (rt_scene_light_visibility); the seed is the render's.
// --light-cone (with --nee or --direct): sphere lights are sampled by solid angle (rt_scene_light_sampling).
// --light-solid-angle (with --nee or --direct): sphere and rect lights are (also when --light-cone is given too).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../../include/shirley_host.h"
#include "../../../include/shirley_rt.h"

namespace {

int verbose = 0;

struct Args {
  std::string scene, output = "out.png", scene_output, scene_input, dump_accum, aspect = "std3x2", bvh = "reference";
  int samples = 100, max_reflect = 50, width = 640, device = 0, sample_chunk = 0, side_len = 11, gpus = 1;
  int partition = RT_PARTITION_AUTO;
  int progressive = 1;
  std::string resume;
  bool adaptive = false;
  double adaptive_threshold = 0.0, noise_floor = 0.01;
  int min_samples = 16, adaptive_step = 16;
  int denoise = -1, denoise_chain = 8;  // --denoise [N]: à-trous iterations (-1: off)
  bool denoise_variance = false;
  double ao = 0.0;  // --ao RADIUS: the ambient-occlusion pass in place of the colour render (0: off)
  int ao_chain = 8;
  bool direct = false;  // --direct: the direct-lighting pass in place of the colour render
  int direct_chain = 8;
  bool nee = false;  // --nee: the light-sampling path integrator in place of the colour render
  int nee_mis = 1;
  bool nee_adaptive = false;  // --nee-adaptive T: rt_render_nee_adaptive in place of rt_render_nee
  double nee_adaptive_threshold = 0.0;
  int light_grid = 0;  // --light-grid N: the light pick of --nee / --direct (0: uniform)
  bool light_grid_given = false;
  int light_visibility = 0;  // --light-visibility K: shadow rays per (cell, light) of the grid (0: off)
  bool light_visibility_given = false;
  bool light_cone = false;  // --light-cone: solid-angle sampling of sphere lights in --nee / --direct
  bool light_solid_angle = false;  // --light-solid-angle: ... of sphere and rect lights
  double fov = 20.0, focal = 1.0, aperture = 0.001;
  bool night = false, single_threaded = false;
  unsigned long long seed = 0x5EED;
};

[[noreturn]] void usage(const char* msg) {
  if (msg && *msg) std::fprintf(stderr, "error: %s\n", msg);
  std::fprintf(stderr,
               "usage: ray-cli [-v] render <random|saved|demo|perlin|earth|box-light|cornell|spheres|final> [options]\n"
               "       ray-cli test\n"
               "options: -o FILE -s N -m N -w N --single-threaded --camera-fov F --camera-focal-length F\n"
               "         --camera-aperture F --camera-aspect-ratio std3x2|std16x9|std16x10|square|target-iphone\n"
               "         --night --scene-output FILE (random)  <scene_input> (saved)  --side-len N (spheres)\n"
               "         --seed N --device N --gpus N --partition tiles|samples --bvh reference|sah --sample-chunk N\n"
               "         --dump-accum FILE --progressive K --resume FILE\n"
               "         --adaptive T --min-samples N --adaptive-step N --noise-floor F\n"
               "         --denoise [N] --denoise-chain K --denoise-variance (with --adaptive)\n"
               "         --ao RADIUS|inf --ao-chain K\n"
               "         --direct --direct-chain K\n"
               "         --nee --nee-mis 0|1\n"
               "         --nee-adaptive T (with --nee; --min-samples N --adaptive-step N --noise-floor F --sample-chunk N)\n"
               "         --light-grid N (with --nee or --direct; 0 ... 64 cells, 0 = uniform pick)\n"
               "         --light-visibility K (with --light-grid N >= 1: 1, 2, 4, 8, 16 or 32 shadow rays per cell and light)\n"
               "         --light-cone (with --nee or --direct: sphere lights sampled by solid angle)\n"
               "         --light-solid-angle (with --nee or --direct: sphere and rect lights sampled by solid angle)\n");
  std::exit(2);
}

// A checkpoint's identity (--dump-accum FILE + FILE.json, --resume FILE): its sums are the per-pixel sums
// of samples [0, samples_done) of one frame, so a resume must render that same frame — the same scene
// (rt_scene_digest_host of the description and BVH builder), camera (FNV-1a over its fields), seed,
// max_depth and sample_chunk (the unit length decides the sums' bits) — and may only add samples.
struct Checkpoint {
  long long samples_done = -1, samples = -1, width = -1, height = -1, max_depth = -1, sample_chunk = -1;
  unsigned long long seed = 0, scene = 0, camera = 0;
};

unsigned long long camera_digest(const rt_camera& c) {
  unsigned long long h = 14695981039346656037ull;
  auto bytes = [&](const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
  };
  bytes(&c.image_width, sizeof c.image_width); bytes(&c.image_height, sizeof c.image_height);
  bytes(&c.height, sizeof c.height); bytes(&c.width, sizeof c.width); bytes(&c.focal_length, sizeof c.focal_length);
  bytes(&c.has_lens, sizeof c.has_lens); bytes(&c.lens_radius, sizeof c.lens_radius);
  bytes(c.origin, sizeof c.origin); bytes(c.w, sizeof c.w); bytes(c.u, sizeof c.u); bytes(c.v, sizeof c.v);
  bytes(&c.focus_length, sizeof c.focus_length); bytes(&c.time0, sizeof c.time0); bytes(&c.time1, sizeof c.time1);
  return h;
}

Checkpoint checkpoint_of(const Args& a, const rt_scene_desc* desc, const rt_camera& cam, int samples, int done) {
  Checkpoint k;
  k.samples_done = done;
  k.samples = samples;
  k.width = cam.image_width;
  k.height = cam.image_height;
  k.max_depth = a.max_reflect;
  k.sample_chunk = a.sample_chunk;
  k.seed = a.seed;
  uint64_t d = 0;
  if (rt_scene_digest_host(desc, a.bvh == "sah" ? RT_BVH_SAH : RT_BVH_REFERENCE, &d) == RT_OK) k.scene = d;
  k.camera = camera_digest(cam);
  return k;
}

void write_checkpoint(const std::string& path, const std::vector<double>& accum, const Checkpoint& k) {
  std::ofstream f(path, std::ios::binary);
  f.write((const char*)accum.data(), (std::streamsize)(accum.size() * sizeof(double)));
  char digests[80];
  std::snprintf(digests, sizeof digests, "\"scene_digest\": \"%016llx\", \"camera_digest\": \"%016llx\"", k.scene,
                k.camera);
  std::ofstream fj(path + ".json");
  fj << "{\"samples_done\": " << k.samples_done << ", \"samples\": " << k.samples << ", \"width\": " << k.width
     << ", \"height\": " << k.height << ", \"seed\": " << k.seed << ", \"max_depth\": " << k.max_depth
     << ", \"sample_chunk\": " << k.sample_chunk << ", " << digests << "}\n";
}

// FILE.json's fields (the writer's own flat format); false when one is missing
bool read_checkpoint(const std::string& path, Checkpoint* k) {
  std::ifstream fj(path + ".json");
  const std::string js((std::istreambuf_iterator<char>(fj)), std::istreambuf_iterator<char>());
  auto field = [&](const char* name, bool hex, unsigned long long* out) {
    const std::string key = std::string("\"") + name + "\":";
    const size_t at = js.find(key);
    if (at == std::string::npos) return false;
    const char* s = js.c_str() + at + key.size();
    while (*s == ' ' || *s == '"') ++s;
    char* end = nullptr;
    *out = std::strtoull(s, &end, hex ? 16 : 10);
    return end != s;
  };
  unsigned long long v[9];
  const char* names[9] = {"samples_done", "samples", "width", "height", "max_depth", "sample_chunk", "seed",
                          "scene_digest", "camera_digest"};
  for (int i = 0; i < 9; ++i)
    if (!field(names[i], i >= 7, &v[i])) return false;
  k->samples_done = (long long)v[0]; k->samples = (long long)v[1]; k->width = (long long)v[2];
  k->height = (long long)v[3]; k->max_depth = (long long)v[4]; k->sample_chunk = (long long)v[5];
  k->seed = v[6]; k->scene = v[7]; k->camera = v[8];
  return true;
}

// Why checkpoint `c` cannot be continued as frame `want` (empty: it can)
std::string checkpoint_mismatch(const Checkpoint& c, const Checkpoint& want) {
  char m[160] = "";
  if (c.scene != want.scene) std::snprintf(m, sizeof m, "scene %016llx, this run %016llx", c.scene, want.scene);
  else if (c.width != want.width || c.height != want.height)
    std::snprintf(m, sizeof m, "%lldx%lld, this run %lldx%lld", c.width, c.height, want.width, want.height);
  else if (c.camera != want.camera) std::snprintf(m, sizeof m, "another camera");
  else if (c.seed != want.seed) std::snprintf(m, sizeof m, "seed %llu, this run %llu", c.seed, want.seed);
  else if (c.max_depth != want.max_depth)
    std::snprintf(m, sizeof m, "max_depth %lld, this run %lld", c.max_depth, want.max_depth);
  else if (c.sample_chunk != want.sample_chunk)
    std::snprintf(m, sizeof m, "sample_chunk %lld, this run %lld", c.sample_chunk, want.sample_chunk);
  else if (c.samples_done < 0 || c.samples_done > want.samples)
    std::snprintf(m, sizeof m, "it covers %lld samples, this run renders %lld", c.samples_done, want.samples);
  return m;
}

// --gpus N > 1: one ctx per device, the scene uploaded to each, rt_render_multi (tiles + RCCL gather
// to the first device), to_image on the host.
int render_scene_multi(const Args& a, const rt_scene_desc* desc, const rt_camera& cam, int samples) {
  std::vector<rt_ctx*> ctxs(a.gpus, nullptr);
  int st = 0;
  auto done = [&](int rc) {
    for (rt_ctx* c : ctxs)
      if (c) rt_destroy(c);
    return rc;
  };
  const int builder = a.bvh == "sah" ? RT_BVH_SAH : RT_BVH_REFERENCE;
  for (int i = 0; i < a.gpus; ++i) {
    if ((st = rt_create(a.device + i, &ctxs[i]))) {
      std::fprintf(stderr, "error: rt_create(device %d) failed (%d)\n", a.device + i, st);
      return done(1);
    }
    if ((st = rt_scene_upload(ctxs[i], desc, builder))) {
      std::fprintf(stderr, "error: %s\n", rt_last_error(ctxs[i]));
      return done(1);
    }
  }
  rt_render_params p{};
  p.samples = samples;
  p.max_depth = a.max_reflect;
  p.seed = a.seed;
  p.tile_world = 1;
  p.sample_chunk = a.sample_chunk;
  p.partition = a.partition;
  const size_t n = (size_t)cam.image_width * cam.image_height * 3;
  std::vector<double> accum(n);
  std::vector<uint8_t> rgb(n);
  auto t1 = std::chrono::steady_clock::now();
  if ((st = rt_render_multi(ctxs.data(), a.gpus, &cam, &p, accum.data()))) {
    std::fprintf(stderr, "error: %s\n", rt_last_error(ctxs[0]));
    return done(1);
  }
  auto t2 = std::chrono::steady_clock::now();
  const double ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
  if (verbose >= 1)
    std::fprintf(stderr, "INFO %d GPUs: render %.1f ms (incl. gather and copy-back): %.1f Msamples/s\n", a.gpus, ms,
                 (double)cam.image_width * cam.image_height * samples / (ms * 1e3));
  rt_tonemap(accum.data(), cam.image_width, cam.image_height, samples, rgb.data());  // image.rs:31-44
  if (!a.dump_accum.empty()) write_checkpoint(a.dump_accum, accum, checkpoint_of(a, desc, cam, samples, samples));
  if (sh_write_png(a.output.c_str(), rgb.data(), cam.image_width, cam.image_height)) {
    std::fprintf(stderr, "error: %s\n", sh_last_error());
    return done(1);
  }
  return done(0);
}

// --denoise: the à-trous filter (rt_denoise_device) between the frame's sums and the tonemap.  The feature
// buffers are rendered over `feature_samples` samples of the frame ([0, feature_samples)); counts (an adaptive
// frame) and variance may be null.  Fills rgb; false on an error (already printed).
struct DevMem {
  std::vector<void*> p;
  ~DevMem() {
    for (void* q : p) (void)hipFree(q);
  }
  template <class T>
  T* get(size_t n, const T* host = nullptr) {
    void* q = nullptr;
    if (hipMalloc(&q, n * sizeof(T)) != hipSuccess) return nullptr;
    p.push_back(q);
    if (host && hipMemcpy(q, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return static_cast<T*>(q);
  }
};

bool denoise_to_rgb(const Args& a, rt_ctx* ctx, const rt_camera& cam, const rt_render_params& frame, int samples,
                    int feature_samples, const double* accum, const int32_t* counts, const double* variance,
                    std::vector<uint8_t>& rgb) {
  const int W = cam.image_width, H = cam.image_height;
  const size_t n_px = (size_t)W * H;
  DevMem mem;
  double* acc_dev = mem.get<double>(n_px * 3, accum);
  double* alb_dev = mem.get<double>(n_px * 3);
  double* nrm_dev = mem.get<double>(n_px * 3);
  double* dep_dev = mem.get<double>(n_px);
  double* out_dev = mem.get<double>(n_px * 3);
  uint8_t* rgb_dev = mem.get<uint8_t>(n_px * 3);
  int32_t* cnt_dev = counts ? mem.get<int32_t>(n_px, counts) : nullptr;
  double* var_dev = variance ? mem.get<double>(n_px, variance) : nullptr;
  if (!acc_dev || !alb_dev || !nrm_dev || !dep_dev || !out_dev || !rgb_dev || (counts && !cnt_dev) ||
      (variance && !var_dev)) {
    std::fprintf(stderr, "error: device allocation of the denoiser's images failed\n");
    return false;
  }
  rt_render_params fp = frame;
  fp.sample_begin = 0;
  fp.sample_count = feature_samples;
  rt_denoise_inputs in{};
  in.width = W;
  in.height = H;
  in.samples = samples;
  in.feature_samples = feature_samples;
  in.accum = acc_dev;
  in.counts = cnt_dev;
  in.albedo = alb_dev;
  in.normal = nrm_dev;
  in.depth = dep_dev;
  in.variance = var_dev;
  rt_denoise_params dp{};  // the documented defaults (include/shirley_rt.h)
  dp.iterations = a.denoise;
  dp.normal_power_log2 = 4;
  dp.sigma_z = 0.05;
  dp.sigma_a = 0.2;
  dp.sigma_c = 2.0;
  dp.albedo_floor = 1e-3;
  int st = rt_render_features_device(ctx, &cam, &fp, a.denoise_chain, alb_dev, nrm_dev, dep_dev, nullptr);
  if (!st) st = rt_denoise_device(ctx, &in, &dp, out_dev, nullptr);
  if (!st)
    st = counts ? rt_tonemap_counts_device(ctx, out_dev, cnt_dev, W, H, rgb_dev, nullptr)
                : rt_tonemap_device(ctx, out_dev, W, H, samples, rgb_dev, nullptr);
  if (!st) st = rt_synchronize(ctx);
  if (st) {
    std::fprintf(stderr, "error: --denoise: %s\n", rt_last_error(ctx));
    return false;
  }
  if (hipMemcpy(rgb.data(), rgb_dev, n_px * 3, hipMemcpyDeviceToHost) != hipSuccess) {
    std::fprintf(stderr, "error: --denoise: copying the picture back failed\n");
    return false;
  }
  return true;
}

int render_scene(const Args& a, const rt_scene_desc* desc, const rt_camera& cam) {
  int samples = a.samples;
  if (samples == 0) {  // main.rs:75-80
    std::fprintf(stderr, "WARN samples set to 0, using 1\n");
    samples = 1;
  }
  if (a.gpus > 1) return render_scene_multi(a, desc, cam, samples);
  if (a.denoise >= 0 || a.ao > 0.0 || a.direct || a.nee)
    for (int i = 0; i < desc->n_objects; ++i) {
      const rt_object& o = desc->objects[i];
      if (o.geometry == RT_GEOM_MOVING_SPHERE || o.medium || o.transform) {
        std::fprintf(stderr, "error: %s: the %s pass does not support book-2 objects (moving spheres, "
                             "media, instance transforms); object %d is one\n",
                     a.nee ? "--nee" : a.direct ? "--direct" : a.ao > 0.0 ? "--ao" : "--denoise",
                     a.nee ? "light-sampling" : a.direct ? "direct-lighting" : a.ao > 0.0 ? "ambient-occlusion" : "feature", i);
        return 1;
      }
    }
  rt_ctx* ctx = nullptr;
  int st = rt_create(a.device, &ctx);
  if (st) {
    std::fprintf(stderr, "error: rt_create(device %d) failed (%d): no usable MI355X device?\n", a.device, st);
    return 1;
  }
  int builder = a.bvh == "sah" ? RT_BVH_SAH : RT_BVH_REFERENCE;
  auto t0 = std::chrono::steady_clock::now();
  if ((st = rt_scene_upload(ctx, desc, builder))) {
    std::fprintf(stderr, "error: %s\n", rt_last_error(ctx));
    rt_destroy(ctx);
    return 1;
  }
  rt_render_params p{};
  p.samples = samples;
  p.max_depth = a.max_reflect;
  p.seed = a.seed;
  p.tile_rank = 0;
  p.tile_world = 1;
  p.sample_chunk = a.sample_chunk;
  const size_t n = (size_t)cam.image_width * cam.image_height * 3;
  std::vector<double> accum;
  std::vector<uint8_t> rgb(n);
  auto t1 = std::chrono::steady_clock::now();
  if (a.ao > 0.0) {
    // the ambient-occlusion pass in place of the colour render: its visibility sums as a grey picture
    std::vector<double> vis(n / 3);
    if ((st = rt_render_ao(ctx, &cam, &p, a.ao_chain, a.ao, vis.data()))) {
      std::fprintf(stderr, "error: --ao: %s\n", rt_last_error(ctx));
      rt_destroy(ctx);
      return 1;
    }
    accum.resize(n);
    for (size_t i = 0; i < n; ++i) accum[i] = vis[i / 3];
    rt_tonemap(accum.data(), cam.image_width, cam.image_height, samples, rgb.data());
    rt_destroy(ctx);
    if (sh_write_png(a.output.c_str(), rgb.data(), cam.image_width, cam.image_height)) {
      std::fprintf(stderr, "error: %s\n", sh_last_error());
      return 1;
    }
    return 0;
  }
  if ((a.direct || a.nee) && a.light_grid > 0 && (st = rt_scene_light_pick(ctx, a.light_grid, nullptr))) {
    std::fprintf(stderr, "error: --light-grid: %s\n", rt_last_error(ctx));
    rt_destroy(ctx);
    return 1;
  }
  if (a.light_visibility > 0) {  // (the argument checks left it with --light-grid N >= 1 and --nee / --direct)
    rt_light_visibility rep;
    if ((st = rt_scene_light_visibility(ctx, a.light_visibility, p.seed, &rep))) {
      std::fprintf(stderr, "error: --light-visibility: %s\n", rt_last_error(ctx));
      rt_destroy(ctx);
      return 1;
    }
    std::fprintf(stderr, "light visibility: %llu shadow rays for %llu cell-light pairs in %.3f ms, %llu unoccluded\n",
                 (unsigned long long)rep.traced, (unsigned long long)rep.pairs, rep.kernel_ms,
                 (unsigned long long)rep.unoccluded);
  }
  if ((a.direct || a.nee) && (a.light_cone || a.light_solid_angle) &&
      (st = rt_scene_light_sampling(ctx, a.light_solid_angle ? (int32_t)RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL
                                                             : (int32_t)RT_LIGHT_SAMPLE_SOLID_ANGLE))) {
    std::fprintf(stderr, "error: %s: %s\n", a.light_solid_angle ? "--light-solid-angle" : "--light-cone",
                 rt_last_error(ctx));
    rt_destroy(ctx);
    return 1;
  }
  if (a.direct) {
    // the direct-lighting pass in place of the colour render: emission + direct through the tonemap
    std::vector<double> direct(n);
    accum.resize(n);
    if ((st = rt_render_direct(ctx, &cam, &p, a.direct_chain, accum.data(), direct.data()))) {
      std::fprintf(stderr, "error: --direct: %s\n", rt_last_error(ctx));
      rt_destroy(ctx);
      return 1;
    }
    for (size_t i = 0; i < n; ++i) accum[i] += direct[i];
    rt_tonemap(accum.data(), cam.image_width, cam.image_height, samples, rgb.data());
    rt_destroy(ctx);
    if (sh_write_png(a.output.c_str(), rgb.data(), cam.image_width, cam.image_height)) {
      std::fprintf(stderr, "error: %s\n", sh_last_error());
      return 1;
    }
    return 0;
  } else if (a.nee) {
    // the light-sampling path integrator in place of the colour render: the same sums, through the tonemap
    accum.resize(n);
    if (a.nee_adaptive) {  // tiles stop at their own sample count, the picture divides by the counts
      rt_adaptive_params ap{};
      ap.min_samples = a.min_samples;
      ap.step = a.adaptive_step;
      ap.threshold = a.nee_adaptive_threshold;
      ap.noise_floor = a.noise_floor;
      std::vector<int32_t> counts(n / 3);
      rt_adaptive_report rep{};
      if ((st = rt_render_nee_adaptive(ctx, &cam, &p, a.nee_mis ? RT_NEE_MIS : 0, &ap, accum.data(), counts.data(),
                                       nullptr, nullptr, &rep))) {
        std::fprintf(stderr, "error: --nee-adaptive: %s\n", rt_last_error(ctx));
        rt_destroy(ctx);
        return 1;
      }
      rt_tonemap_counts(accum.data(), counts.data(), cam.image_width, cam.image_height, rgb.data());
      rt_destroy(ctx);
      if (verbose >= 1)
        std::fprintf(stderr, "INFO adaptive: %d steps, mean %.2f spp of at most %d, %.1f %% of %d tiles converged\n",
                     rep.steps, (double)rep.samples / (double)(n / 3), samples,
                     100.0 * rep.tiles_converged / (double)(rep.tiles ? rep.tiles : 1), rep.tiles);
      if (sh_write_png(a.output.c_str(), rgb.data(), cam.image_width, cam.image_height)) {
        std::fprintf(stderr, "error: %s\n", sh_last_error());
        return 1;
      }
      return 0;
    }
    if ((st = rt_render_nee(ctx, &cam, &p, a.nee_mis ? RT_NEE_MIS : 0, accum.data()))) {
      std::fprintf(stderr, "error: --nee: %s\n", rt_last_error(ctx));
      rt_destroy(ctx);
      return 1;
    }
    rt_tonemap(accum.data(), cam.image_width, cam.image_height, samples, rgb.data());
    rt_destroy(ctx);
    if (sh_write_png(a.output.c_str(), rgb.data(), cam.image_width, cam.image_height)) {
      std::fprintf(stderr, "error: %s\n", sh_last_error());
      return 1;
    }
    return 0;
  } else if (a.adaptive) {
    // adaptive sampling: tiles stop at their own sample count, the picture divides by the counts
    rt_adaptive_params ap{};
    ap.min_samples = a.min_samples;
    ap.step = a.adaptive_step;
    ap.threshold = a.adaptive_threshold;
    ap.noise_floor = a.noise_floor;
    accum.resize(n);
    std::vector<int32_t> counts(n / 3);
    rt_adaptive_report rep{};
    std::vector<double> moments(a.denoise_variance ? n / 3 * 2 : 0), variance(a.denoise_variance ? n / 3 : 0);
    if ((st = rt_render_adaptive(ctx, &cam, &p, &ap, accum.data(), counts.data(),
                                 a.denoise_variance ? moments.data() : nullptr, nullptr, &rep))) {
      std::fprintf(stderr, "error: %s\n", rt_last_error(ctx));
      rt_destroy(ctx);
      return 1;
    }
    if (a.denoise >= 0) {
      // the features come from the samples every pixel holds, [0, min_samples); the counts from the call
      if (a.denoise_variance)
        rt_moments_variance(moments.data(), counts.data(), a.sample_chunk ? a.sample_chunk : 4, cam.image_width,
                            cam.image_height, variance.data());
      if (!denoise_to_rgb(a, ctx, cam, p, samples, a.min_samples, accum.data(), counts.data(),
                          a.denoise_variance ? variance.data() : nullptr, rgb)) {
        rt_destroy(ctx);
        return 1;
      }
    } else {
      rt_tonemap_counts(accum.data(), counts.data(), cam.image_width, cam.image_height, rgb.data());
    }
    if (verbose >= 1)
      std::fprintf(stderr, "INFO adaptive: %d steps, mean %.2f spp of at most %d, %.1f %% of %d tiles converged\n",
                   rep.steps, (double)rep.samples / (double)(n / 3), samples,
                   100.0 * rep.tiles_converged / (double)(rep.tiles ? rep.tiles : 1), rep.tiles);
  } else if (a.progressive > 1 || !a.resume.empty()) {
    // progressive rendering with checkpoints: sample ranges [b_k, b_k+1) of the frame; the host adds each
    // range's sums to the running sums in range order (so a resumed run adds exactly what an
    // uninterrupted one does) and writes the checkpoint after every range
    accum.assign(n, 0.0);
    int done = 0;
    if (!a.resume.empty()) {
      Checkpoint ck;
      if (!read_checkpoint(a.resume, &ck)) {
        std::fprintf(stderr, "error: %s.json is not a checkpoint record\n", a.resume.c_str());
        rt_destroy(ctx);
        return 1;
      }
      const std::string why = checkpoint_mismatch(ck, checkpoint_of(a, desc, cam, samples, 0));
      if (!why.empty()) {
        std::fprintf(stderr, "error: %s is a checkpoint of another frame: %s\n", a.resume.c_str(), why.c_str());
        rt_destroy(ctx);
        return 1;
      }
      std::ifstream f(a.resume, std::ios::binary);
      f.read((char*)accum.data(), (std::streamsize)(n * sizeof(double)));
      if (!f || f.gcount() != (std::streamsize)(n * sizeof(double)) || f.peek() != std::char_traits<char>::eof()) {
        std::fprintf(stderr, "error: %s does not hold the %zu sums of a %dx%d frame\n", a.resume.c_str(), n,
                     cam.image_width, cam.image_height);
        rt_destroy(ctx);
        return 1;
      }
      done = (int)ck.samples_done;
    }
    std::vector<double> part(n);
    const int ranges = std::max(1, a.progressive);
    const int left = samples - done;
    for (int k = 0; k < ranges && left > 0; ++k) {
      const int b = done + (int)((long long)left * k / ranges), e = done + (int)((long long)left * (k + 1) / ranges);
      if (e <= b) continue;
      p.sample_begin = b;
      p.sample_count = e - b;
      if ((st = rt_render(ctx, &cam, &p, part.data()))) {
        std::fprintf(stderr, "error: %s\n", rt_last_error(ctx));
        rt_destroy(ctx);
        return 1;
      }
      for (size_t i = 0; i < n; ++i) accum[i] += part[i];
      rt_tonemap(accum.data(), cam.image_width, cam.image_height, e, rgb.data());
      if (!a.dump_accum.empty()) write_checkpoint(a.dump_accum, accum, checkpoint_of(a, desc, cam, samples, e));
      if (sh_write_png(a.output.c_str(), rgb.data(), cam.image_width, cam.image_height)) {
        std::fprintf(stderr, "error: %s\n", sh_last_error());
        rt_destroy(ctx);
        return 1;
      }
      if (verbose >= 1) std::fprintf(stderr, "INFO checkpoint: samples [0, %d) of %d\n", e, samples);
    }
    rt_destroy(ctx);
    if (left == 0) {  // a complete checkpoint: just its picture
      rt_tonemap(accum.data(), cam.image_width, cam.image_height, samples, rgb.data());
      if (sh_write_png(a.output.c_str(), rgb.data(), cam.image_width, cam.image_height)) {
        std::fprintf(stderr, "error: %s\n", sh_last_error());
        return 1;
      }
    }
    return 0;
  } else if (!a.dump_accum.empty() || a.denoise >= 0) {  // the raw sums are wanted on the host: render + host tonemap
    accum.resize(n);
    if ((st = rt_render(ctx, &cam, &p, accum.data()))) {
      std::fprintf(stderr, "error: %s\n", rt_last_error(ctx));
      rt_destroy(ctx);
      return 1;
    }
    if (a.denoise >= 0) {  // features over the frame's samples, filter, tonemap: all on the device
      if (!denoise_to_rgb(a, ctx, cam, p, samples, samples, accum.data(), nullptr, nullptr, rgb)) {
        rt_destroy(ctx);
        return 1;
      }
    } else {
      rt_tonemap(accum.data(), cam.image_width, cam.image_height, samples, rgb.data());  // image.rs:31-44
    }
  } else {  // sums stay in HBM; to_image runs on the device and only RGB8 crosses PCIe
    double* acc_dev = nullptr;
    uint8_t* rgb_dev = nullptr;
    if (hipMalloc((void**)&acc_dev, n * sizeof(double)) != hipSuccess || hipMalloc((void**)&rgb_dev, n) != hipSuccess) {
      std::fprintf(stderr, "error: device allocation of the image failed\n");
      rt_destroy(ctx);
      return 1;
    }
    st = rt_render_device(ctx, &cam, &p, acc_dev, nullptr);
    if (!st) st = rt_tonemap_device(ctx, acc_dev, cam.image_width, cam.image_height, samples, rgb_dev, nullptr);
    if (!st) st = rt_synchronize(ctx);
    if (!st && hipMemcpy(rgb.data(), rgb_dev, n, hipMemcpyDeviceToHost) != hipSuccess) st = RT_E_HIP;
    (void)hipFree(acc_dev);
    (void)hipFree(rgb_dev);
    if (st) {
      std::fprintf(stderr, "error: %s\n", rt_last_error(ctx));
      rt_destroy(ctx);
      return 1;
    }
  }
  auto t2 = std::chrono::steady_clock::now();
  rt_counters cnt{};
  rt_counters_get(ctx, &cnt);
  double ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
  double msamp = (double)cam.image_width * cam.image_height * samples / (cnt.kernel_ms * 1e3);
  if (verbose >= 1 && !a.adaptive)  // (an adaptive frame printed its own line: the counters hold its last step)
    std::fprintf(stderr,
                 "INFO upload %.1f ms, render %.1f ms (kernel %.2f ms, reduce %.3f ms): %.1f Msamples/s, %.3f segments/sample\n",
                 std::chrono::duration<double, std::milli>(t1 - t0).count(), ms, cnt.kernel_ms, cnt.reduce_ms, msamp,
                 (double)cnt.segments / (double)(cnt.samples ? cnt.samples : 1));
  rt_destroy(ctx);
  if (!a.dump_accum.empty())  // a complete checkpoint
    write_checkpoint(a.dump_accum, accum, checkpoint_of(a, desc, cam, samples, samples));
  if (sh_write_png(a.output.c_str(), rgb.data(), cam.image_width, cam.image_height)) {
    std::fprintf(stderr, "error: %s\n", sh_last_error());
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    std::string s = argv[i];
    auto next = [&]() -> std::string {
      if (i + 1 >= argc) usage(("missing value for " + s).c_str());
      return argv[++i];
    };
    if (s == "-v" || s == "--verbose") ++verbose;
    else if (s.size() > 2 && s[0] == '-' && s[1] == 'v' && s.find_first_not_of('v', 1) == std::string::npos) verbose += (int)s.size() - 1;
    else if (s == "-o" || s == "--output") a.output = next();
    else if (s == "-s" || s == "--samples") a.samples = std::atoi(next().c_str());
    else if (s == "-m" || s == "--max-reflect") a.max_reflect = std::atoi(next().c_str());
    else if (s == "--single-threaded") a.single_threaded = true;
    else if (s == "-w" || s == "--width") a.width = std::atoi(next().c_str());
    else if (s == "--camera-fov") a.fov = std::atof(next().c_str());
    else if (s == "--camera-focal-length") a.focal = std::atof(next().c_str());
    else if (s == "--camera-aperture") a.aperture = std::atof(next().c_str());
    else if (s == "--camera-aspect-ratio") a.aspect = next();
    else if (s == "--night") a.night = true;
    else if (s == "--scene-output") a.scene_output = next();
    else if (s == "--seed") a.seed = std::strtoull(next().c_str(), nullptr, 0);
    else if (s == "--device") a.device = std::atoi(next().c_str());
    else if (s == "--gpus") a.gpus = std::atoi(next().c_str());
    else if (s == "--bvh") a.bvh = next();
    else if (s == "--sample-chunk") a.sample_chunk = std::atoi(next().c_str());
    else if (s == "--progressive") a.progressive = std::atoi(next().c_str());
    else if (s == "--resume") a.resume = next();
    else if (s == "--adaptive") { a.adaptive = true; a.adaptive_threshold = std::atof(next().c_str()); }
    else if (s == "--min-samples") a.min_samples = std::atoi(next().c_str());
    else if (s == "--adaptive-step") a.adaptive_step = std::atoi(next().c_str());
    else if (s == "--noise-floor") a.noise_floor = std::atof(next().c_str());
    else if (s == "--denoise") {  // the iteration count is optional: taken when the next argument is a number
      a.denoise = 3;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') a.denoise = std::atoi(argv[++i]);
    }
    else if (s == "--denoise-chain") a.denoise_chain = std::atoi(next().c_str());
    else if (s == "--denoise-variance") a.denoise_variance = true;
    else if (s == "--ao") {  // a radius > 0; strtod reads `inf`
      a.ao = std::strtod(next().c_str(), nullptr);
      if (!(a.ao > 0.0)) usage("--ao takes a radius > 0 (or inf)");
    }
    else if (s == "--ao-chain") a.ao_chain = std::atoi(next().c_str());
    else if (s == "--direct") a.direct = true;
    else if (s == "--direct-chain") a.direct_chain = std::atoi(next().c_str());
    else if (s == "--nee") a.nee = true;
    else if (s == "--nee-adaptive") { a.nee_adaptive = true; a.nee_adaptive_threshold = std::atof(next().c_str()); }
    else if (s == "--nee-mis") {
      const std::string v = next();
      a.nee_mis = v == "0" ? 0 : v == "1" ? 1 : -1;
    }
    else if (s == "--light-grid") {
      a.light_grid = std::atoi(next().c_str());
      a.light_grid_given = true;
    }
    else if (s == "--light-visibility") {
      a.light_visibility = std::atoi(next().c_str());
      a.light_visibility_given = true;
    }
    else if (s == "--light-cone") a.light_cone = true;
    else if (s == "--light-solid-angle") a.light_solid_angle = true;
    else if (s == "--partition") {
      const std::string v = next();
      if (v == "tiles") a.partition = RT_PARTITION_TILES;
      else if (v == "samples") a.partition = RT_PARTITION_SAMPLES;
      else usage("--partition must be tiles or samples");
    }
    else if (s == "--dump-accum") a.dump_accum = next();
    else if (s == "--side-len") a.side_len = std::atoi(next().c_str());
    else if (s == "-h" || s == "--help") usage("");
    else if (!s.empty() && s[0] == '-') usage(("unknown option " + s).c_str());
    else pos.push_back(s);
  }
  if (pos.empty()) usage("missing subcommand");
  if (pos[0] == "test") {  // main.rs:60-63
    std::fprintf(stderr, "ERROR there is nothing to test!\n");
    return 0;
  }
  if (pos[0] != "render" || pos.size() < 2) usage("expected `render <scene>`");
  a.scene = pos[1];
  if (a.samples < 0 || a.max_reflect < 0 || a.width < 1) usage("samples / max-reflect / width out of range");
  if (a.gpus < 1 || a.gpus > 64) usage("--gpus must be in [1, 64]");
  if (a.progressive < 1) usage("--progressive must be >= 1");
  if (a.gpus > 1 && (a.progressive > 1 || !a.resume.empty())) usage("--progressive / --resume render on one GPU");

  if (a.nee_adaptive && !a.nee) usage("--nee-adaptive sets the stop rule of --nee");
  if (a.nee_adaptive && (a.gpus > 1 || a.progressive > 1 || !a.resume.empty() || !a.dump_accum.empty()))
    usage("--nee-adaptive renders on one GPU, without --progressive / --resume / --dump-accum");
  if (a.nee_adaptive && (a.adaptive || a.denoise >= 0 || a.ao > 0.0 || a.direct))
    usage("--nee-adaptive is --nee's own stop rule: no --adaptive, no --denoise, no --ao, no --direct");
  if (a.nee && (a.gpus > 1 || a.progressive > 1 || !a.resume.empty()))
    usage("--nee renders on one GPU, without --progressive / --resume");
  if (a.nee && (a.adaptive || a.denoise >= 0 || a.ao > 0.0 || a.direct))
    usage("--nee replaces the colour render: no --adaptive, no --denoise, no --ao, no --direct");
  if (a.nee && !a.dump_accum.empty()) usage("--nee frames are not checkpointed (--dump-accum)");
  if (a.nee_mis != 0 && a.nee_mis != 1) usage("--nee-mis 0 or 1");

  if (a.adaptive && (a.gpus > 1 || a.progressive > 1 || !a.resume.empty()))
    usage("--adaptive renders on one GPU, without --progressive / --resume");
  if (a.adaptive && !a.dump_accum.empty()) usage("--adaptive frames are not checkpointed (--dump-accum)");

  if (a.denoise >= 0 && (a.gpus > 1 || a.progressive > 1 || !a.resume.empty()))
    usage("--denoise filters a frame rendered on one GPU, without --progressive / --resume");
  if (a.denoise > 8 || a.denoise_chain < 0) usage("--denoise takes 0 to 8 iterations, --denoise-chain K >= 0");
  if (a.denoise_variance && !(a.adaptive && a.denoise >= 0))
    usage("--denoise-variance feeds the moments of an --adaptive frame to --denoise");

  if (a.ao > 0.0 && (a.gpus > 1 || a.progressive > 1 || !a.resume.empty()))
    usage("--ao renders on one GPU, without --progressive / --resume");
  if (a.ao > 0.0 && (a.adaptive || a.denoise >= 0)) usage("--ao replaces the colour render: no --adaptive, no --denoise");
  if (a.ao > 0.0 && !a.dump_accum.empty()) usage("--ao frames are not checkpointed (--dump-accum)");
  if (a.ao_chain < 0) usage("--ao-chain K >= 0");

  if (a.direct && (a.gpus > 1 || a.progressive > 1 || !a.resume.empty()))
    usage("--direct renders on one GPU, without --progressive / --resume");
  if (a.direct && (a.adaptive || a.denoise >= 0 || a.ao > 0.0))
    usage("--direct replaces the colour render: no --adaptive, no --denoise, no --ao");
  if (a.direct && !a.dump_accum.empty()) usage("--direct frames are not checkpointed (--dump-accum)");
  if (a.direct_chain < 0) usage("--direct-chain K >= 0");

  if (a.light_cone && !(a.nee || a.direct)) usage("--light-cone sets the light sampling of --nee or --direct");
  if (a.light_solid_angle && !(a.nee || a.direct))
    usage("--light-solid-angle sets the light sampling of --nee or --direct");
  if (a.light_grid_given && !(a.nee || a.direct)) usage("--light-grid sets the light pick of --nee or --direct");
  if (a.light_grid < 0 || a.light_grid > 64) usage("--light-grid N in 0 ... 64");
  if (a.light_visibility_given) {
    const int k = a.light_visibility;
    if (!(k == 1 || k == 2 || k == 4 || k == 8 || k == 16 || k == 32)) usage("--light-visibility K in 1, 2, 4, 8, 16, 32");
    if (!(a.nee || a.direct) || a.light_grid < 1)
      usage("--light-visibility weights the grid of --light-grid N (N >= 1) with --nee or --direct");
  }

  sh_scene* scene = nullptr;
  std::string cam_scene = a.scene;
  if (a.scene == "saved") {
    if (pos.size() < 3) usage("render saved needs <scene_input>");
    std::ifstream f(pos[2]);
    if (!f) usage(("cannot open " + pos[2]).c_str());
    std::stringstream ss;
    ss << f.rdbuf();
    if (sh_scene_from_json(ss.str().c_str(), &scene)) {
      std::fprintf(stderr, "error: %s\n", sh_last_error());
      return 1;
    }
  } else {
    std::string name = a.scene;
    if (name == "random" && a.night) name = "random-night";
    if (name == "spheres") name = "spheres:" + std::to_string(a.side_len);
    if (sh_scene_builtin(name.c_str(), a.seed, &scene)) {
      std::fprintf(stderr, "error: %s\n", sh_last_error());
      return 1;
    }
  }
  if (!a.scene_output.empty()) {  // scenes.rs:140-143
    size_t need = 0;
    sh_scene_to_json(scene, 1, nullptr, 0, &need);
    std::string buf(need, '\0');
    sh_scene_to_json(scene, 1, &buf[0], need, &need);
    std::ofstream f(a.scene_output);
    f << buf.c_str();
  }
  sh_desc* desc = nullptr;
  if (sh_scene_finalize(scene, a.seed, &desc)) {
    std::fprintf(stderr, "error: %s\n", sh_last_error());
    return 1;
  }
  rt_camera cam{};
  if (sh_scene_camera(cam_scene.c_str(), a.width, a.aspect.c_str(), a.fov, a.focal, a.aperture, &cam)) {
    std::fprintf(stderr, "error: %s\n", sh_last_error());
    return 1;
  }
  int rc = render_scene(a, sh_desc_view(desc), cam);
  sh_desc_free(desc);
  sh_scene_free(scene);
  return rc;
}
