/*
 * shirley_rt.h — drop-in C ABI for the reference's render hot path on MI355X.
 *
 * What this replaces (all paths relative to scottschroeder/shirley-raytracing-rs):
 *   - src/main.rs:65-130        render_scene(): the rayon loop over scanlines (main.rs:92-126)
 *   - src/raytracer/render.rs:49-70  render_scanline(frame, rng, samples, max_depth, ws, line_idx, buf)
 *   - src/raytracer/render.rs:17-48  ray_color()  (the per-sample bounce loop)
 *   - src/raytracer/scene/mod.rs:111-137  SceneBuilder::finalize (texture load + BBox tree build)
 *
 * A host (the C++ host in this repo, or a Rust crate binding this header verbatim with
 * bindgen/#[repr(C)]) owns the scene description, the camera and the
 * image buffer.  The library owns device memory.  Everything here is plain C: fixed-width
 * integers, doubles, raw pointers and sizes.  No C++ types and no exceptions cross this ABI.
 *
 * Arithmetic is IEEE binary64 throughout, like the reference (core/math.rs:5 `type Real = f64`).
 *
 * Errors: every entry point returns an rt_status; rt_last_error(ctx) holds a message.
 * Threading: one rt_ctx per device; a ctx must not be used from two host threads at once.
 */
#ifndef SHIRLEY_RT_H
#define SHIRLEY_RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 11

typedef enum rt_status {
  RT_OK = 0,
  RT_E_INVALID = 1,     /* bad argument / malformed scene */
  RT_E_HIP = 2,         /* HIP runtime error (no device, launch failure, ...) */
  RT_E_OOM = 3,         /* device allocation failed */
  RT_E_UNSUPPORTED = 4, /* feature not compiled in / not available */
  RT_E_RCCL = 5         /* RCCL (librccl) missing or a collective failed (multi-GPU entry points) */
} rt_status;

/* geometry/object.rs:9-16  GeometricObject */
enum { RT_GEOM_SPHERE = 0, RT_GEOM_RECT_XY = 1, RT_GEOM_RECT_YZ = 2, RT_GEOM_RECT_XZ = 3, RT_GEOM_RECT_BOX = 4,
       /* book-2 ("The Next Week") extension, absent from the reference:
        * a sphere whose centre moves linearly from p[0..2] at q[3] to q[0..2] at q[4] */
       RT_GEOM_MOVING_SPHERE = 5 };
/* material/material_type.rs:20-27  MaterialType */
enum { RT_MAT_METAL = 0, RT_MAT_DIELECTRIC = 1, RT_MAT_LAMBERTIAN = 2, RT_MAT_DIFFUSE_LIGHT = 3, RT_MAT_FAIRY_LIGHT = 4,
       /* book-2 extension (absent from the reference): the phase function of a ConstantMedium —
        * scatters to random_in_unit_sphere() with the texture's albedo */
       RT_MAT_ISOTROPIC = 5 };
/* material/texture/loader.rs:17-28  TextureLoader (after load: Solid / Checker / Noise / Image) */
enum { RT_TEX_SOLID = 0, RT_TEX_CHECKER = 1, RT_TEX_PERLIN = 2, RT_TEX_IMAGE = 3 };
/* skybox/mod.rs:11-16  SkyBox */
enum { RT_SKY_ABOVE = 0, RT_SKY_FLAT = 1, RT_SKY_NONE = 2 };
/* BVH builder selection for rt_scene_upload */
enum {
  RT_BVH_REFERENCE = 0, /* bvh/bbox_tree/constructor.rs split rules (median/midpoint on min-x/y/z, volume score) */
  RT_BVH_SAH = 1,       /* surface-area heuristic, exact sweep over every object boundary (performance option; the same hits:
                           exact ties in t go to the reference tree's winner whichever tree is walked) */
  /* node placement flags OR-ed into the builder argument (testing / tuning) */
  RT_BVH_NODES_GLOBAL = 0x100,   /* every node read through L1/L2 (the default) */
  RT_BVH_NODES_HALF_LDS = 0x200, /* top half of the nodes copied into LDS per block (mixed path) */
  RT_BVH_NODES_LDS = 0x400       /* as many nodes in LDS as fit next to the traversal stacks */
};
/* Trace engine for rt_render_params.engine.  Both compute the same ray_color() arithmetic and give
 * the same pixels; they differ only in how the bounce loop is scheduled on the GPU. */
enum {
  RT_ENGINE_AUTO = 0,       /* the faster engine on MI355X (today: the megakernel; env SHIRLEY_ENGINE overrides) */
  RT_ENGINE_MEGAKERNEL = 1, /* one persistent kernel runs whole paths, lane-level path regeneration */
  RT_ENGINE_WAVEFRONT = 2,  /* extend / shade / texture kernels over a pool of path slots in HBM;
                             * the host loop blocks until the frame is traced */
  RT_ENGINE_SPLIT = 3,      /* ABI 5: the megakernel with its traversal decoupled from its shading
                             * (one block per CU: shading waves post rays to traversal waves through
                             * LDS queues).  Scenes that fit it: reference primitives only, whole scene
                             * in LDS; otherwise the call falls back to RT_ENGINE_MEGAKERNEL and
                             * rt_counters.engine says so */
  RT_ENGINE_TIMING = 0x10   /* flag: time every kernel launch with HIP events (rt_counters *_ms) */
};

/* One scene object = SceneLoadObject{geometry, material} (scene/mod.rs:23-27).
 * The fields after p[] are book-2 ("The Next Week") extensions that the reference does not have
 * (SURVEY.md §0.1 config 5); all zero = a reference object.  Their semantics are DESIGN.md §10's
 * (parity unpinned: no reference implementation exists). */
typedef struct rt_object {
  int32_t geometry; /* RT_GEOM_* */
  int32_t material; /* index into rt_scene_desc.materials */
  /* Sphere  (geometry/sphere.rs:11-15): cx cy cz radius (radius may be negative: sphere.rs:48,54-60)
   * Rect    (geometry/rect.rs:45-52):   d1_min d1_max d2_min d2_max offset
   * RectBox (geometry/rect.rs:102-130): min.x min.y min.z max.x max.y max.z (sides derived as RectBox::new)
   * MovingSphere: center0 xyz, radius */
  double p[6];
  int32_t medium;     /* 1: a ConstantMedium whose boundary is this geometry (material: RT_MAT_ISOTROPIC) */
  int32_t transform;  /* 1: instance transform, world = Translate(offset) . RotateY(rotate_y_deg) . object */
  double q[5];        /* MovingSphere: center1 xyz, time0, time1 */
  double density;     /* ConstantMedium density (neg_inv_density = -1/density) */
  double rotate_y_deg;
  double offset[3];
} rt_object;

typedef struct rt_material {
  int32_t kind;      /* RT_MAT_* */
  int32_t texture;   /* albedo texture (Lambertian / DiffuseLight / FairyLight), -1 otherwise */
  double albedo[3];  /* Metal albedo (metal.rs:10-14) */
  double param;      /* Metal: fuzz, already clamped <= 1 (metal.rs:17-23); Dielectric: ir (dielectric.rs:10-13) */
} rt_material;

typedef struct rt_texture {
  int32_t kind;      /* RT_TEX_* */
  int32_t odd;       /* Checker: odd child texture index  (checker.rs:10-14) */
  int32_t even;      /* Checker: even child texture index */
  int32_t table;     /* Perlin: index into perlin tables; Image: index into images */
  double color[3];   /* Solid colour (solid.rs:5-21) */
  double scale;      /* Checker: size; Perlin: scale (perlin/mod.rs:143-153) */
} rt_texture;

/* Perlin tables (perlin/mod.rs:11-17): 256 non-normalised random vectors + 3 permutations. */
typedef struct rt_perlin_table {
  double ranfloat[256][3];
  int32_t perm_x[256];
  int32_t perm_y[256];
  int32_t perm_z[256];
} rt_perlin_table;

/* Decoded RGB8 image texture (image_texture.rs:15-17); row 0 = top, like image::DynamicImage. */
typedef struct rt_image {
  int32_t width;
  int32_t height;
  const uint8_t* rgb; /* width*height*3 bytes */
} rt_image;

/* Flattened SceneBuilder (scene/mod.rs:79-83) with textures already "loaded" and deduplicated
 * (TextureManager::load, texture/loader.rs:113-131).  Host-owned; borrowed for the call only. */
typedef struct rt_scene_desc {
  int32_t sky;            /* RT_SKY_* */
  double sky_color[3];    /* RT_SKY_FLAT colour */
  int32_t n_objects;
  const rt_object* objects;
  int32_t n_materials;
  const rt_material* materials;
  int32_t n_textures;
  const rt_texture* textures;
  int32_t n_perlin;
  const rt_perlin_table* perlin;
  int32_t n_images;
  const rt_image* images;
} rt_scene_desc;

/* Camera (camera/mod.rs:88-95) + CameraPosition (camera/mod.rs:63-70), as built by
 * CameraBuilder::build (camera/mod.rs:44-60) and CameraPosition::look_at (camera/mod.rs:72-86),
 * with the caller's `pos.focus_length = 10.0` override already applied (scenes.rs:209,229). */
typedef struct rt_camera {
  int32_t image_width;   /* Dimmensions.width */
  int32_t image_height;  /* Dimmensions.height */
  double height;         /* 2 tan(vfov/2) */
  double width;          /* aspect * height */
  double focal_length;
  int32_t has_lens;      /* lens_radius: Option<f64> */
  double lens_radius;
  double origin[3];
  double w[3], u[3], v[3];
  double focus_length;
  /* shutter interval (book-2 extension, absent from the reference): a path's ray time is
   * time0 + (time1 - time0) * U, U from its own counter-RNG stream; only moving spheres read it */
  double time0, time1;
} rt_camera;

/* Per-call render parameters (RenderSettings, argparse.rs:106-123, plus what the reference lacks). */
typedef struct rt_render_params {
  int32_t samples;      /* samples per pixel; 0 is treated as 1 (main.rs:75-80) */
  int32_t max_depth;    /* max_reflect: bounce limit of ray_color (render.rs:30) */
  uint64_t seed;        /* key of the counter-based RNG (the reference is unseeded: SURVEY.md §0) */
  int32_t tile_rank;    /* interleaved 8x8-tile sharding: this call renders tiles k with k % tile_world == tile_rank */
  int32_t tile_world;   /* 1 = whole frame */
  int32_t sample_chunk; /* samples per work unit (0 = automatic; >= samples gives in-order per-pixel sums).
                         * Automatic usually picks chunk < samples: each chunk is summed in order, then the
                         * chunk sums in chunk order — not render.rs:58-69's single running sum, so the
                         * frame differs from the in-order one by reassociation only (|d| <= 1e-12 |sum|,
                         * DESIGN.md §2).  The megakernel indexes a launch's work units (pixels x chunks) in 32 bits: a
                         * call with more runs in several sample passes (see scratch_mb).
                         * The automatic length depends on the pixels a call renders (its tiles) and on
                         * the device's CU count, so tile-sharded frames at different world sizes sum each
                         * pixel's chunks differently (bits differ within the reassociation bound); pass an
                         * explicit sample_chunk for frames that are bit-identical at every world size. */
  int32_t engine;       /* RT_ENGINE_* (0 = automatic), optionally | RT_ENGINE_TIMING */
  /* ABI 6: the call's sample range — SURVEY.md §8(b)'s "sample range" — and its scratch bound.
   * The call renders samples [sample_begin, sample_begin + sample_count) of every pixel (0 <= sample_begin,
   * range within [0, samples)); sample_count == 0 means "to samples".  The output holds the sums over the
   * range only.  The counter RNG is keyed by the global sample index, so ranges [0, k) and [k, S) render
   * exactly the samples of one [0, S) call (the pixel sums differ by reassociation only: the per-pixel
   * sum of two ranges is (sum of range 1) + (sum of range 2)).  Reference: render.rs:58-69's sample loop. */
  int32_t sample_begin;
  int32_t sample_count;
  /* multi-GPU entry points (rt_render_sharded / rt_render_multi): how the frame is split over the ranks,
   * RT_PARTITION_*; ignored by the single-device calls */
  int32_t partition;
  /* bound on the per-call partial-sum scratch in MiB (0 = default 8192).  A call whose [chunks][pixels][3]
   * f64 partial sums exceed it renders its chunks in consecutive sample passes, each reduced into the
   * output in chunk order — the same per-pixel additions in the same order as one pass, so the frame is
   * bit-identical for every bound. */
  int32_t scratch_mb;
} rt_render_params;

/* ABI 6: rt_render_params.partition (multi-GPU) */
enum {
  RT_PARTITION_AUTO = 0,    /* the measured default per world size */
  RT_PARTITION_TILES = 1,   /* interleaved 8x8 tiles (tile k -> rank k % world), gather of the packed tiles to
                             * rank 0: every pixel's sum is computed on one rank, so the frame equals the
                             * single-device frame whenever the unit length (sample_chunk) is the same */
  RT_PARTITION_SAMPLES = 2  /* every rank renders all pixels for its share of the sample range (rank r:
                             * [count*r/world, count*(r+1)/world) of it); the per-rank sums are exchanged by
                             * row bands (all-to-all), summed in rank order and gathered to rank 0:
                             * deterministic, equal to the single-device frame within reassociation */
};

typedef struct rt_scene_stats {
  int32_t n_objects;
  int32_t n_nodes;      /* BVH nodes (leaves included), like BboxTree.tree.len()+... */
  int32_t n_leaves;
  int32_t depth;        /* max root-to-leaf depth */
  int64_t device_bytes; /* scene bytes resident in HBM */
  /* ABI 4: the renderer's collapsed tree (the one rt_render* and RT_TRAVERSAL_RENDER walk) */
  int32_t n_nodes4;     /* 4-wide f32 nodes */
  int32_t wide_block;   /* 1: the trace kernel keeps the whole 4-wide tree in LDS (1024-thread blocks) */
  double origin_limit;  /* rays with max|origin| above this take the f64 re-test of the f32 node boxes */
  /* ABI 9 */
  int32_t hop_pass;     /* 1: the trace kernel runs its hop pass (a reference scene held in LDS with a dielectric
                         * RectBox; SHIRLEY_NO_HOP at upload: 0); frames and counters are the same either way */
  /* added within ABI 11, in the struct's former tail padding: its size stays 48 bytes and every earlier field keeps
   * its offset, so RT_ABI_VERSION is unchanged (a caller built before it reads what it read) */
  int32_t hop_kind;     /* how the hop pass finds a candidate's closest hit: 0 no pass, 1 a visit of the tree's first
                         * node, 2 the scene's ground stack alone (its rects and RectBoxes under spheres that rest on
                         * them; SHIRLEY_HOP=root at upload: 1 where 2 would be chosen) */
} rt_scene_stats;

/* Counters of the last render call (deterministic for a given seed). */
typedef struct rt_counters {
  uint64_t samples;     /* paths started = pixels x spp */
  uint64_t segments;    /* ray_color loop iterations that traced a ray (hit + miss) */
  uint64_t node_visits; /* BVH child-box tests (4-wide trees: 4 per node visit); the 4-wide traversal of the
                         * megakernel / wavefront counts them only in the instrumented build (-DRT_PHASE_TIMING,
                         * DESIGN.md §5): 0 otherwise */
  uint64_t prim_tests;  /* primitive intersection calls (same condition) */
  double kernel_ms;     /* device time of the trace (all trace kernels of the frame, HIP events) */
  double reduce_ms;     /* device time of the partial-sum reduce kernel */
  int32_t engine;       /* RT_ENGINE_MEGAKERNEL, RT_ENGINE_WAVEFRONT or RT_ENGINE_SPLIT: the engine that ran */
  int32_t iterations;   /* wavefront: extend/shade/texture rounds (0 for the megakernel) */
  uint64_t slots;       /* wavefront: path slots in flight */
  double extend_ms;     /* wavefront + RT_ENGINE_TIMING: summed device time of wf_extend launches */
  double shade_ms;      /* ... wf_shade launches */
  double texture_ms;    /* ... wf_texture launches */
  int32_t sample_chunk; /* ABI 4: samples per work unit the call used (auto-sized when params.sample_chunk == 0;
                         * < samples means each pixel's sum is added up per chunk, then chunk sums in order) */
  int32_t n_chunks;     /* ceil(samples / sample_chunk) */
  /* ABI 6 */
  int32_t passes;        /* sample passes the call used (> 1 when the partial sums exceed scratch_mb) */
  int32_t trace_launches;/* trace-kernel launches of the call (one per pass; kernel_ms is their summed time) */
  uint64_t scratch_bytes;/* partial-sum scratch the call used */
} rt_counters;

typedef struct rt_ctx rt_ctx;

/* ---- library / device ---------------------------------------------------------------------- */
const char* rt_version(void);
int rt_device_count(int32_t* out);
int rt_create(int32_t device, rt_ctx** out);
int rt_destroy(rt_ctx* ctx);
const char* rt_last_error(const rt_ctx* ctx);

/* ---- scene (replaces SceneBuilder::finalize, scene/mod.rs:111-137) --------------------------- */
int rt_scene_upload(rt_ctx* ctx, const rt_scene_desc* scene, int32_t bvh_builder);
int rt_scene_stats_get(rt_ctx* ctx, rt_scene_stats* out);
/* Added within ABI 11 (purely additive): which megakernel instance the uploaded scene's hop pass runs — 0 none,
 * 1 the first-node visit, 2 the ground stack's pass, 3 the same with the down pass before the sampler, 4 both by the
 * closed-form next plane of a plane stack (a ground stack whose y planes lie a gap apart inside a common xz core;
 * SHIRLEY_HOP=general at upload: 3 where 4 would be chosen).  rt_scene_stats.hop_kind is 2 for 2, 3 and 4: frames
 * and counters are the same under every instance. */
int rt_scene_hop_instance(rt_ctx* ctx, int32_t* out);
/* ABI 6: 64-bit digest of the uploaded scene (its description and BVH builder; FNV-1a over every field),
 * and the same digest computed on the host from a description (no device needed).  Equal scenes give
 * equal digests; the multi-GPU calls compare them across ranks. */
int rt_scene_digest(rt_ctx* ctx, uint64_t* out);
int rt_scene_digest_host(const rt_scene_desc* scene, int32_t bvh_builder, uint64_t* out);

/* ---- rendering (replaces main.rs:92-126 + render.rs:17-70) ----------------------------------- */
/* Whole frame, blocking.  accum_host: [image_height][image_width][3] f64 per-pixel SUMS over the
 * samples (Image.data layout, image.rs:10-14), row 0 = bottom of the picture (image.rs:38). */
int rt_render(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params, double* accum_host);

/* Rows [line_begin, line_end) only, blocking — the render_scanline (render.rs:49-57) granularity.
 * rows_host: [(line_end-line_begin)][image_width][3] sums; samples of row j identical to rt_render's. */
int rt_render_scanlines(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params,
                        int32_t line_begin, int32_t line_end, double* rows_host);

/* Device-resident variants: asynchronous on `stream` (a hipStream_t, NULL = the ctx's own stream).
 * rt_render_device: accum_dev is [H][W][3] f64 in HBM; pixels of tiles not owned by this
 * (tile_rank, tile_world) are left untouched.
 * rt_render_tiles_device: packed output [n_tiles_rank][8][8][3] f64 (tile-local row 0 = lowest row),
 * for the multi-GPU gather; rt_unpack_tiles_device scatters a gathered [world][max_tiles][8][8][3]
 * buffer back into [H][W][3]. */
int rt_tile_layout(const rt_camera* cam, int32_t tile_world, int32_t* n_tiles_total, int32_t* max_tiles_per_rank);
int rt_render_device(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params, double* accum_dev,
                     void* stream);
int rt_render_tiles_device(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params,
                           double* packed_dev, void* stream);
int rt_unpack_tiles_device(rt_ctx* ctx, const rt_camera* cam, int32_t tile_world, const double* gathered_dev,
                           double* accum_dev, void* stream);
int rt_synchronize(rt_ctx* ctx);

/* Closest hit for a batch of rays, blocking — Hittable for Scene (scene/mod.rs:180-190) /
 * WorkspaceScene::hit_workspace (scene/mod.rs:152-164).  rays: [n][6] = origin xyz, direction xyz.
 * out[i].object = -1 on a miss; otherwise the HitRecord (geometry/hittable.rs:6-14) of object index. */
typedef struct rt_hit {
  int32_t object;
  int32_t front_face;
  double t;
  double point[3];
  double normal[3];
  double u, v;
} rt_hit;
int rt_scene_hit(rt_ctx* ctx, const double* rays, int32_t n, double t_min, double t_max, rt_hit* out);

/* ABI 4: the same query through a chosen traversal.
 *   RT_TRAVERSAL_BINARY: the 2-wide f64 tree (the reference's BboxTree as built; what rt_scene_hit walks);
 *   RT_TRAVERSAL_RENDER: the traversal the trace kernel runs — the 4-wide collapsed tree with conservative
 *     f32 (inflated) child boxes, exact f64 leaf re-tests and an f64 fallback for rays whose origin lies
 *     beyond rt_scene_stats.origin_limit, with nodes and primitives read from where the renderer reads them.
 * Both return the reference's closest hit (bbox_tree.rs:56-91 + hit2 + the object tests). */
enum { RT_TRAVERSAL_BINARY = 0, RT_TRAVERSAL_RENDER = 1 };
int rt_scene_hit_ex(rt_ctx* ctx, const double* rays, int32_t n, double t_min, double t_max, int32_t traversal,
                    rt_hit* out);

/* ABI 7: one iteration of ray_color's loop (render.rs:30-46) for each given ray, through the megakernel's
 * own device code — the render traversal (t in [0.001, inf)), the hit record, the material and its texture
 * (Perlin marble evaluated by the wave), the wave's sampler for the scatter's draws, and the shading —
 * with ray i on the path key (seed, pixel = i, sample, draw): emitted() and scatter() of the hit's material
 * (material_type.rs:51-79), or the sky on a miss (skybox/mod.rs:5-25), and the path's draw counter after
 * the segment.  A verification probe of the scatter semantics (tests/test_scatter_kat.py); book-2 ray time 0. */
typedef struct rt_probe {
  int32_t object;          /* closest object, -1: missed (the sky) */
  int32_t front_face;
  int32_t scattered;       /* scatter() returned Some: the path goes on along (origin, direction) */
  int32_t emits;           /* emitted() returned Some (or the sky): `emitted` holds it */
  uint32_t draw;           /* the path's draw counter after the segment */
  int32_t pad;
  double t, point[3], normal[3];
  double emitted[3];
  double attenuation[3];   /* scatter().attenuation */
  double origin[3], direction[3];  /* scatter().direction: the next ray */
} rt_probe;
int rt_probe_segment(rt_ctx* ctx, const double* rays, int32_t n, uint64_t seed, uint32_t sample, uint32_t draw,
                     rt_probe* out);

/* ---- multi-GPU (ABI 4) -------------------------------------------------------
 * The frame's 8x8 tiles are dealt round-robin over the ranks of a communicator (tile k -> rank
 * k % world); each rank renders its tiles into a packed buffer and RCCL gathers the packed buffers to
 * rank 0 over xGMI (ncclGather), which scatters them into the [H][W][3] image (RT_PARTITION_TILES), or
 * every rank renders all pixels for a share of the samples (RT_PARTITION_SAMPLES, see above).  The
 * counter RNG is keyed by the global pixel and sample, so a tile-sharded frame is bit-identical for every
 * world size given an explicit sample_chunk (the automatic chunk follows the rank's pixel count).  Every
 * ctx must hold the same scene and every rank must pass the same call arguments: every call of
 * rt_render_sharded all-gathers each rank's (scene digest, call key) — the key hashes the resolved partition
 * and sample range, samples, seed, max_depth, sample_chunk and the camera — so all ranks issue the same
 * collective sequence whatever their arguments, and checks the gathered words on the host: in the call,
 * before any collective of the frame, when this rank's key differs from the one the ranks last agreed on
 * (ranks changing scene or arguments together all fail there with RT_E_INVALID on a mismatch); otherwise
 * at the rank's next call, so a loop of frames needs no host round trip.  Misuse — one rank changing its
 * key alone — fails that rank in the call; its peers have already issued the frame's collectives, which it
 * never joins, so their stream waits (undefined from RCCL's side: do not rely on it).  A failed check poisons
 * the communicator: every later rt_render_sharded call on it returns RT_E_INVALID and issues no collective
 * (a new all-gather could otherwise be paired with a peer's pending frame collective); destroy it with
 * rt_comm_destroy and create a new one.  SHIRLEY_KEY_CHECK=sync
 * checks every call before the frame's collectives (every rank fails in the call itself, one host round
 * trip per call).  rt_render_multi compares the digests on the host.  Replaces the
 * reference's whole-machine rayon loop over scanlines (main.rs:92-126).  RCCL is loaded on first use
 * (dlopen "librccl.so.1": the copy already in the process if any); without it these calls return
 * RT_E_RCCL.
 *
 * One process per GPU: rank 0 calls rt_comm_unique_id, hands the id to every rank by any channel
 * (torch.distributed's store, MPI, a file), and each rank calls rt_comm_init_rank on its own ctx.
 * One process driving several GPUs: rt_render_multi (communicators created and cached per ctx set). */
#define RT_COMM_ID_BYTES 128
typedef struct rt_comm rt_comm;
int rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES]);
int rt_comm_init_rank(rt_ctx* ctx, const uint8_t id[RT_COMM_ID_BYTES], int32_t world, int32_t rank, rt_comm** out);
int rt_comm_destroy(rt_comm* comm);
/* One rank's share of a sharded frame, asynchronous on `stream` (NULL: the ctx's stream) after the
 * cross-rank check above: render the rank's share (params->partition: its tiles, or all pixels for its samples;
 * params->tile_rank / tile_world are ignored: the communicator's rank and size are used), exchange, and on
 * rank 0 write accum_dev ([H][W][3] f64 sums on its device; NULL on the other ranks).  The sample range of
 * params (sample_begin / sample_count) is the frame's; a sample partition splits it.  Every rank of the
 * communicator must make the call (a collective). */
int rt_render_sharded(rt_ctx* ctx, rt_comm* comm, const rt_camera* cam, const rt_render_params* params,
                      double* accum_dev, void* stream);
/* The whole frame on n devices from one process, blocking; accum_host as rt_render's ([H][W][3] sums, row
 * 0 = bottom).  ctxs[0] is the root; every ctx needs the same scene uploaded (the digests are compared
 * first: RT_E_INVALID on a mismatch).  params->partition as rt_render_sharded's.  n == 1 equals rt_render. */
int rt_render_multi(rt_ctx* const* ctxs, int32_t n, const rt_camera* cam, const rt_render_params* params,
                    double* accum_host);

/* Counters (segments etc.) of the most recent render call; blocks until it finished. */
int rt_counters_get(rt_ctx* ctx, rt_counters* out);

/* Host-only BVH inspection (no device needed): builds the tree rt_scene_upload would build.
 * Call with nodes = NULL to get *n_nodes, then again with room for that many.  Node layout follows
 * BboxTree.tree (bbox_tree.rs:10-26): leaf >= 0 is the object index, else lhs/rhs are node indices. */
typedef struct rt_bvh_node {
  double box[6]; /* min xyz, max xyz */
  int32_t leaf;
  int32_t lhs, rhs;
  int32_t pad;
} rt_bvh_node;
int rt_bvh_build_host(const rt_scene_desc* scene, int32_t bvh_builder, int32_t* n_nodes, rt_bvh_node* nodes,
                      int32_t* root);

/* Output stage on the host, exactly image::to_image (image.rs:31-44) + Color::to_pixel (color.rs:31-38):
 * c/samples -> sqrt -> (x*255.999) saturating to u8, row j -> output row H-1-j.  rgb8: [H][W][3], row 0 = top. */
int rt_tonemap(const double* accum, int32_t width, int32_t height, int32_t samples, uint8_t* rgb8);
/* The same on the device: accum_dev [H][W][3] sums -> rgb8_dev [H][W][3] with
 * row 0 = top, on `stream` (NULL: the context's stream), asynchronous.  Bit-identical to rt_tonemap. */
int rt_tonemap_device(rt_ctx* ctx, const double* accum_dev, int32_t width, int32_t height, int32_t samples,
                      uint8_t* rgb8_dev, void* stream);

/* ---- adaptive sampling (ABI 8) -------------------------------------------------
 * One frame in steps: every pixel gets min_samples, then steps of `step` more samples go only to the
 * 8x8 tiles whose noise estimate is still above the threshold, up to params->samples per pixel.  The
 * counter RNG is keyed by the global (pixel, sample), so a pixel that stops after n samples holds exactly
 * samples [0, n) of the uniform frame: its sums equal rt_render's over sample range [0, n) with the same
 * sample_chunk bit for bit.
 *
 * A batch is params->sample_chunk consecutive samples of a pixel (b; 0 means 4) and y = (r + g) + b of a
 * batch's sum one observation; a pixel's moments are m1 = sum y, m2 = sum y^2 over its n batches.  A
 * tile's error over its K in-image pixels after N = n b samples per pixel:
 *   v_p = max(0, m2_p - m1_p^2 / n) / (n - 1),  E = sum_p v_p,  M = sum_p m1_p,
 *   e = sqrt(n E / K) / (M / K + N noise_floor)        (e = 0 when E == 0)
 * — the RMS standard error of the tile's pixel means relative to the tile's mean r + g + b.  After each
 * step a tile goes on while !(e <= threshold): a NaN error keeps rendering.  Threshold 0 stops no tile (also
 * none with e == 0), so that frame is rt_render's; +inf stops every tile with a finite error at min_samples. */
typedef struct rt_adaptive_params {
  int32_t min_samples;   /* every pixel gets these first; a multiple of the batch, >= 2 batches */
  int32_t step;          /* samples per later step; a multiple of the batch */
  double  threshold;     /* a tile stops when its error e <= threshold; 0 = never, +inf = at min_samples */
  double  noise_floor;   /* per-sample r+g+b added to the tile mean in e's denominator */
} rt_adaptive_params;

typedef struct rt_adaptive_report {
  int32_t  steps, tiles, tiles_converged, pad; /* steps run; tiles of the frame; tiles the rule stopped */
  uint64_t samples, segments;      /* paths and segments traced, summed over the steps */
  double   kernel_ms, fold_ms;     /* device time of the trace launches / of the rest (fold kernels), summed */
} rt_adaptive_report;

/* Whole frame, blocking.  params->samples is the per-pixel maximum; samples, min_samples and step must be
 * multiples of the batch; sample_begin, sample_count must be 0 and tile_world 1 (RT_E_INVALID otherwise).
 * The megakernel renders the steps' tile lists: RT_ENGINE_AUTO resolves to it, RT_ENGINE_WAVEFRONT and
 * RT_ENGINE_SPLIT return RT_E_UNSUPPORTED.  scratch_mb bounds each step's partial sums as in rt_render; the
 * frame is bit-identical for every bound.  max_depth == 0 gives zero sums and every tile stops at
 * min_samples.  Not available through the multi-GPU entry points; adaptive frames are not checkpointed. */
int rt_render_adaptive(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params,
                       const rt_adaptive_params* adaptive,
                       double* accum_host,      /* [H][W][3] sums over each pixel's own samples, row 0 = bottom */
                       int32_t* counts_host,    /* [H][W] samples the pixel received */
                       double* moments_host,    /* [H][W][2] m1, m2; may be NULL */
                       double* tile_error_host, /* [tiles] e at the tile's last check, tile k = 8x8 tile
                                                   (k % tiles_x, k / tiles_x) from the bottom row; may be NULL */
                       rt_adaptive_report* report /* may be NULL */);

/* rt_tonemap with each pixel's own count in place of `samples` (counts: [H][W], accum's row order); a count
 * of 0 gives black.  Uniform counts give rt_tonemap's bytes.  The device variant is asynchronous on `stream`
 * (NULL: the context's stream) and bit-identical to the host one. */
int rt_tonemap_counts(const double* accum, const int32_t* counts, int32_t width, int32_t height, uint8_t* rgb8);
int rt_tonemap_counts_device(rt_ctx* ctx, const double* accum_dev, const int32_t* counts_dev, int32_t width,
                             int32_t height, uint8_t* rgb8_dev, void* stream);

/* ---- feature buffers and the à-trous denoiser (ABI 10) ----------------------------
 * Feature buffers: per-pixel SUMS over the call's sample range of the albedo, the normal and the depth seen
 * along each sample's own path — the auxiliary images a reconstruction filter is guided by.  Sample s of
 * pixel p runs on the render's path key (seed, p, s): the render's camera ray (jitter draws 0 and 1, then
 * the lens-disk draws), then the render's own dielectric segments.
 *   depth   the camera ray's closest-hit t in [0.001, inf); 0 on a miss.
 *   chain   the path is followed while its closest hit is RT_MAT_DIELECTRIC and fewer than `chain` dielectric
 *           vertices have been followed (chain >= 0; 0 = the first hit).  Each step is exactly the renderer's
 *           dielectric segment — the same draw index, odd-half cache and Schlick decision — i.e. what
 *           rt_probe_segment returns when called with the path's running draw counter.
 *   feature vertex (where the chain stops)
 *           miss: albedo = the sky colour of that ray (rt_probe.emitted), normal = 0;
 *           hit:  normal = the hit record's normal; albedo = rt_material.albedo (Metal), (1, 1, 1)
 *           (Dielectric: chain exhausted), else the material's texture value at the record's (u, v, point)
 *           (Lambertian, DiffuseLight, FairyLight: no direction factor, no normalisation).
 * params->samples, seed, sample_begin and sample_count mean what they mean for rt_render; tile_world must be
 * 1; max_depth, engine, sample_chunk and scratch_mb are ignored.  Samples are added in order.
 * albedo / normal: [H][W][3] f64, depth: [H][W] f64, row 0 = bottom; any of the three may be NULL.
 * Scenes with book-2 objects return RT_E_UNSUPPORTED (a ray's first hit in a medium is a random variable).
 * rt_render_features blocks; rt_render_features_device takes device pointers and is asynchronous on `stream`
 * (NULL: the context's stream), like rt_render_device. */
int rt_render_features(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params, int32_t chain,
                       double* albedo_host, double* normal_host, double* depth_host);
int rt_render_features_device(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params, int32_t chain,
                              double* albedo_dev, double* normal_dev, double* depth_dev, void* stream);

/* The filter: an edge-aware à-trous wavelet filter (Dammertz et al. 2010) on the albedo-demodulated frame.
 * With c, a, n, z the per-pixel means (sums / their sample counts) and A = max(a, albedo_floor) per channel:
 *   prepare    c^ = c / A per channel;  var^ = variance / ((A_r^2 + A_g^2 + A_b^2) / 3)
 *   iterations i = 0 .. iterations-1 with stride s = 2^i over the 5x5 taps h = (1/16, 1/4, 3/8, 1/4, 1/16) x h
 *              at offsets s (dx, dy), dy = -2..2 outer, dx = -2..2 inner, taps outside the image skipped:
 *                c^'_p = sum_q h_q w_pq c^_q / sum_q h_q w_pq
 *                var^'_p = sum_q (h_q w_pq)^2 var^_q / (sum_q h_q w_pq)^2
 *              w_pp = 1;  w_pq = ((w_n w_z) w_a) w_c for q != p, with f(x) = max(0, 1 - x)^2:
 *                w_n  1 when |n_p|^2 = |n_q|^2 = 0 (both sky), 0 when exactly one is 0, else
 *                     max(0, n_p.n_q)^2 / (|n_p|^2 |n_q|^2) squared normal_power_log2 times (4: cos^32)
 *                w_z  f(r^2), r = (z_p - z_q) / (sigma_z (z_p + z_q) + 1e-300)
 *                w_a  f(|a_p - a_q|^2 / sigma_a^2)
 *                w_c  f(|c^_p - c^_q|^2 / (sigma_c^2 (var^_p + var^_q) + 1e-300)) on the iteration's input
 *                     values; 1 when `variance` is NULL
 *   finish     out = (c^ A) count
 * Only + - * /, comparisons and selects in a fixed order (no libm, no fused multiply-add): the device result
 * equals the host's bit for bit.  A pixel whose c^ is not finite is copied through unchanged and has weight 0
 * as a neighbour; a pixel with count 0 outputs 0 and is not used as a neighbour.  iterations == 0 returns
 * the input sums.  Defaults (the Python binding's and ray-cli's): iterations 3, normal_power_log2 4,
 * sigma_z 0.05, sigma_a 0.2, sigma_c 2, albedo_floor 1e-3.  RT_E_INVALID: iterations outside [0, 8],
 * normal_power_log2 outside [0, 16], a sigma or the floor not > 0, a negative count, samples < 1 without
 * counts, feature_samples < 1, a NULL accum / albedo / normal / depth. */
typedef struct rt_denoise_inputs {
  int32_t width, height;
  int32_t samples;          /* every pixel's sample count when counts == NULL */
  int32_t feature_samples;  /* samples summed in albedo / normal / depth */
  const double* accum;      /* [H][W][3] sums (rt_render / rt_render_adaptive), row order as theirs */
  const int32_t* counts;    /* [H][W] per-pixel sample counts (an adaptive frame), or NULL */
  const double* albedo;     /* [H][W][3] sums (rt_render_features) */
  const double* normal;     /* [H][W][3] sums */
  const double* depth;      /* [H][W] sums */
  const double* variance;   /* [H][W] variance of the pixel's MEAN r + g + b, or NULL: no colour term */
} rt_denoise_inputs;

typedef struct rt_denoise_params {
  int32_t iterations;         /* [0, 8]; stride 2^i in iteration i */
  int32_t normal_power_log2;  /* [0, 16] */
  double sigma_z, sigma_a, sigma_c;
  double albedo_floor;
} rt_denoise_params;

/* out_sums: [H][W][3] on the input's scale (filtered mean x the pixel's count): rt_tonemap / rt_tonemap_counts
 * apply unchanged.  rt_denoise runs on the host and needs no device; rt_denoise_device takes device pointers
 * in `in` and out_sums_dev, is asynchronous on `stream` (NULL: the context's stream) and uses scratch of its
 * own kept on the context (a negative count is not diagnosed there: such a pixel is treated as count 0). */
int rt_denoise(const rt_denoise_inputs* in, const rt_denoise_params* params, double* out_sums);
int rt_denoise_device(rt_ctx* ctx, const rt_denoise_inputs* in, const rt_denoise_params* params,
                      double* out_sums_dev, void* stream);

/* rt_render_adaptive's moments ([H][W][2] m1, m2 over batches of `batch` samples) and counts ([H][W]) to the
 * filter's variance input: out[p] = v_p n / N^2 with n = counts[p] / batch batches, N = counts[p] samples and
 * v_p the batch-means variance above (NaN for n < 2).  Host and device (asynchronous on `stream`) forms. */
int rt_moments_variance(const double* moments, const int32_t* counts, int32_t batch, int32_t width, int32_t height,
                        double* out);
int rt_moments_variance_device(rt_ctx* ctx, const double* moments_dev, const int32_t* counts_dev, int32_t batch,
                               int32_t width, int32_t height, double* out_dev, void* stream);

/* ---- occlusion queries and the ambient-occlusion pass (ABI 11) ---------------------
 * Any-hit query: out[i] = 1 iff some object is hit by ray i with t in [t_min, tmax_i], tmax_i = t_max_each ?
 * t_max_each[i] : t_max — exactly when rt_scene_hit_ex(RT_TRAVERSAL_RENDER) on [t_min, tmax_i] reports
 * object >= 0; else 0.  The walk is the render traversal's with its accept decisions unchanged, but it never
 * shrinks t_max and ends on the first accepted object.  A per-ray bound is what a shadow ray needs: the
 * distance to the light.  Rays are finite with non-zero directions.  n == 0 is RT_OK.  RT_E_INVALID: a NULL
 * rays or out, n < 0, a NaN t_min or t_max, no scene uploaded.  Scenes with book-2 objects return
 * RT_E_UNSUPPORTED (a medium's hit is a random variable, a moving sphere needs a ray time).
 * rt_scene_occluded blocks; rt_scene_occluded_device takes device pointers and is asynchronous on `stream`
 * (NULL: the context's stream), like rt_render_features_device. */
int rt_scene_occluded(rt_ctx* ctx, const double* rays /* [n][6] */, int32_t n, double t_min, double t_max,
                      const double* t_max_each /* [n] or NULL */, uint8_t* out /* [n] */);
int rt_scene_occluded_device(rt_ctx* ctx, const double* rays_dev, int32_t n, double t_min, double t_max,
                             const double* t_max_each_dev, uint8_t* out_dev, void* stream);

/* Ambient occlusion: per-pixel SUMS over the call's sample range of a 0/1 visibility ([H][W] f64, row 0 =
 * bottom).  Sample s of pixel p runs on the render's path key (seed, p, s): rt_render_features's camera ray
 * and dielectric chain (the same `chain` >= 0) to the feature vertex, where the path's draw counter is D.
 *   miss       visibility 1.
 *   direction  the renderer's Lambertian scatter at that record, whatever the material: r =
 *              random_in_unit_sphere on draws D, D+1, ...; w = normal + unit(r), or normal where w is near
 *              zero (lambertian.rs:21-37) — at a Lambertian vertex the render's own next ray, bit for bit.
 *   occlusion  t_max = radius / |w| (radius = +inf: +inf); visibility 0 iff the ray (point, w) is occluded
 *              on [0.001, t_max] in the sense of rt_scene_occluded, else 1.
 * params->samples, seed, sample_begin and sample_count mean what they mean for rt_render_features;
 * tile_world must be 1; the other fields are ignored.  radius must be > 0 or +inf.  RT_E_INVALID: a NaN,
 * zero or negative radius, a negative chain, tile_world != 1, a bad sample range, a NULL output.  Scenes
 * with book-2 objects return RT_E_UNSUPPORTED.  rt_render_ao blocks; rt_render_ao_device takes a device
 * pointer and is asynchronous on `stream` (NULL: the context's stream). */
int rt_render_ao(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params, int32_t chain, double radius,
                 double* ao_host /* [H][W] */);
int rt_render_ao_device(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params, int32_t chain,
                        double radius, double* ao_dev, void* stream);

/* ---- the scene's light list and the direct-lighting pass ---------------------------
 * Added within ABI 11, as rt_scene_stats.hop_kind was: the entry points below are purely additive — no
 * earlier struct, enum or function changes — so RT_ABI_VERSION stays 11.
 *
 * Light list.  A listed light is an object, neither medium nor instance (medium == transform == 0), whose
 * material is RT_MAT_DIFFUSE_LIGHT or RT_MAT_FAIRY_LIGHT with an RT_TEX_SOLID texture and whose geometry is
 *   RT_GEOM_RECT_XY / YZ / XZ with d1_max - d1_min > 0 and d2_max - d2_min > 0, or
 *   RT_GEOM_SPHERE with radius > 0.
 * Lights are listed in object order.  Every other object with one of the two emitter materials — a checker,
 * Perlin or image texture, a RectBox, a moving sphere, a zero or negative radius, an empty rect, a medium or
 * an instance — is unlisted: counted, and seen by the pass below only when a camera path lands on it.
 *   area   rect: (d1_max - d1_min) * (d2_max - d2_min);  sphere: (4 * pi) * (r * r), pi = 3.141592653589793
 *          (IEEE binary64 products in this order). */
typedef struct rt_light {
  int32_t object;    /* index into rt_scene_desc.objects */
  int32_t geometry;  /* RT_GEOM_* of that object */
  int32_t emitter;   /* RT_MAT_DIFFUSE_LIGHT or RT_MAT_FAIRY_LIGHT */
  int32_t pad;
  double area;
  double color[3];   /* the solid texture's colour */
} rt_light;
/* The uploaded scene's list (built by rt_scene_upload) / the same list from a description, without a device.
 * *n_lights and *n_unlisted (either may be NULL) receive the counts; out == NULL asks for the counts only,
 * otherwise it has room for *n_lights records. */
int rt_scene_lights(rt_ctx* ctx, int32_t* n_lights, int32_t* n_unlisted, rt_light* out);
int rt_scene_lights_host(const rt_scene_desc* scene, int32_t* n_lights, int32_t* n_unlisted, rt_light* out);

/* Direct lighting: per-pixel SUMS over the call's sample range of what the feature vertex emits (`emission`)
 * and of a one-light-sample estimate of the light reaching it from the listed lights (`direct`); both
 * [H][W][3] f64, row 0 = bottom; either may be NULL, not both.  Sample s of pixel p runs on the render's path
 * key (seed, p, s): rt_render_features's camera ray and dielectric chain (the same `chain` >= 0) to the feature
 * vertex, where the path's draw counter is D, the hit record is (x, n) and the last ray's direction is d.
 *   emission  what rt_probe_segment reports as `emitted` there when `emits`: the sky on a miss, the texture
 *             value of a DiffuseLight, texture value * (dot(n, -d) / |d|) of a FairyLight (any texture kind);
 *             0 otherwise.
 *   direct    0 unless the vertex is Lambertian or FairyLight and the scene lists L >= 1 lights.  With `a` the
 *             renderer's scatter attenuation there (rt_probe.attenuation: the texture value, unit(value) for a
 *             FairyLight), on the path's draws D, D+1, ...:
 *     pick      xi0 = draw D;  k = min((int)(xi0 * (double)L), L - 1): light k of the list.
 *               (With a light grid set by rt_scene_light_pick, below: k = the smallest index with xi0 < cdf_k in
 *               the row of x's cell, p = cdf_k - (k ? cdf_(k-1) : 0.0).)
 *     rect      xi1, xi2 = draws D+1, D+2;  y[d1] = d1_min + xi1 * (d1_max - d1_min),
 *               y[d2] = d2_min + xi2 * (d2_max - d2_min), y[axis] = offset, with (d1, d2, axis) = (x, y, z) for
 *               RECT_XY, (y, z, x) for RECT_YZ, (x, z, y) for RECT_XZ (geometry/rect.rs).
 *     sphere    r = random_in_unit_sphere on draws D+1, ... (three per attempt; each coordinate -1 + 2 * draw,
 *               accepted when (x*x + y*y) + z*z <= 1);  u = r / sqrt((x*x + y*y) + z*z) per component;
 *               y = c + radius * u.
 *     geometry  w = y - x;  d2 = (w.x*w.x + w.y*w.y) + w.z*w.z;  dist = sqrt(d2);
 *               cx = ((n.x*w.x + n.y*w.y) + n.z*w.z) / dist;
 *               cy = |w[axis]| / dist for a rect (the reference's emitters radiate from both faces),
 *               cy = -((u.x*w.x + u.y*w.y) + u.z*w.z) / dist for a sphere (far-side area samples count zero).
 *     cut       !(cx > 0 && cy > 0): the sample contributes 0 and no shadow ray is traced (a NaN fails too).
 *     shadow    the sample contributes 0 iff the ray (x, w) is occluded on [0.001, 1 - 2^-20] in the sense of
 *               rt_scene_occluded.  The interval stops short of the light itself: an occluder closer to the
 *               light than 2^-20 of the distance between vertex and light sample is ignored.
 *     value     Le = colour (DiffuseLight) or colour * cy per channel (FairyLight; lighting.rs:59-65 for the ray
 *               (x, w));  g = ((cx * cy) / d2) * ((area * (double)L) / pi);  direct_c = (a_c * Le_c) * g.
 *               (With a light grid: g = ((cx * cy) / d2) * ((area / p) / pi).)
 *   Only + - * /, a correctly rounded sqrt, comparisons and selects, in the order written (no fused
 *   multiply-add): a restatement in IEEE binary64 gives the same bits wherever `a` needs no libm function.
 *   The light sample's density is 1 / (L * area) per unit area, so E[direct] is the vertex's exact direct
 *   illumination from the listed lights times `a`, and emission + direct has the expectation of rt_render
 *   with max_depth = 2 where every emitter is listed and the sky is RT_SKY_NONE.
 * params->samples, seed, sample_begin and sample_count mean what they mean for rt_render_ao; tile_world must
 * be 1; the other fields are ignored.  Samples are added in order.  RT_E_INVALID: both outputs NULL, a
 * negative chain, tile_world != 1, a bad sample range.  Scenes with book-2 objects return RT_E_UNSUPPORTED.
 * rt_render_direct blocks; rt_render_direct_device takes device pointers and is asynchronous on `stream`
 * (NULL: the context's stream). */
int rt_render_direct(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params, int32_t chain,
                     double* emission_host /* [H][W][3] or NULL */, double* direct_host /* [H][W][3] or NULL */);
int rt_render_direct_device(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params, int32_t chain,
                            double* emission_dev, double* direct_dev, void* stream);

/* ---- the light-sampling path integrator --------------------------------------------
 * Added within ABI 11 like the light list: purely additive, RT_ABI_VERSION stays 11.
 *
 * rt_render_nee is rt_render's path with one light sample (the estimator of rt_render_direct above) at every
 * Lambertian / FairyLight vertex, and a weight on the emission that the vertex's own scatter then lands on.
 * Output: rt_render's layout — [H][W][3] f64 SUMS over the call's sample range, row 0 = bottom; rt_tonemap and
 * rt_denoise apply unchanged.  params->samples, max_depth, seed, sample_begin and sample_count mean what they
 * mean for rt_render; tile_world must be 1; engine, sample_chunk and scratch_mb are ignored.  Each pixel's
 * samples are added in order.  max_depth <= 0 gives zero sums.
 *
 * Sample s of pixel p runs on the render's path key (seed, p, s) and starts with the render's camera ray.
 * Segments are numbered k = 1 ... max_depth; att = (1, 1, 1), rad = (0, 0, 0); L = the number of listed
 * lights.  Segment k does what rt_probe_segment returns for the current ray when called with the path's
 * running draw counter: the closest hit on [0.001, inf), the record (t, point, n_hit, front_face), `emitted`,
 * and `scatter` (attenuation a, next ray (x, d')) on the renderer's own draws.
 *   miss        rad += att * sky (per channel); the path ends.  A sky is never listed.
 *   emission    a hit that emits: rad += (att * emitted) * ws (per channel, in this order), where
 *               listed(hit) = the hit object is light j of the list, and it is a rect or the hit is front_face;
 *               ws = 1 unless the previous vertex took a light sample and listed(hit);
 *               if both hold and RT_NEE_MIS is clear: ws = 0;
 *               if both hold and RT_NEE_MIS is set, with d the segment's ray direction and t its hit parameter:
 *                 ld2 = (d.x*d.x + d.y*d.y) + d.z*d.z;  ld = sqrt(ld2);
 *                 cy = -((n_hit.x*d.x + n_hit.y*d.y) + n_hit.z*d.z) / ld;  d2 = (t*t) * ld2;
 *                 gs = ((cx_prev * cy) / d2) / pi;  pl = 1.0 / (area_j * (double)L);  ws = gs / (pl + gs);
 *                 ws = 1 when !(cx_prev > 0 && cy > 0).
 *               (A sphere light seen from inside: light sampling gives such a vertex nothing, cy <= 0 there, so
 *               the scatter keeps that emission in full.)
 *   no scatter  the path ends.
 *   light       taken iff the vertex material is Lambertian or FairyLight, L >= 1 and k < max_depth (it stands
 *   sample      for segment k + 1's emission, so the last vertex takes none), on the path's draws after the
 *               scatter's own: rt_render_direct's estimator at (x, n) = the record with a = the scatter
 *               attenuation — the same pick, rect or sphere sample, w, d2, dist, cx, cy, the cut
 *               !(cx > 0 && cy > 0) before any ray, the shadow ray (x, w) on [0.001, 1 - 2^-20], Le.
 *               value_c = (a_c * Le_c) * g with
 *                 RT_NEE_MIS clear: g = ((cx * cy) / d2) * ((area * (double)L) / pi);
 *                 RT_NEE_MIS set:   gs = ((cx * cy) / d2) / pi;  pl = 1.0 / (area * (double)L);  g = gs / (pl + gs).
 *               (With a light grid set by rt_scene_light_pick, below: the grid's pick, and
 *                 RT_NEE_MIS clear: g = ((cx * cy) / d2) * ((area / p) / pi);
 *                 RT_NEE_MIS set:   pl = p / area, here and, with p_j(cell_prev), in `emission` above.)
 *               rad += att * value (per channel).  Remembered for the next hit: that a sample was taken (cut and
 *               occluded ones included) and cx_prev = ((n.x*d'.x + n.y*d'.y) + n.z*d'.z) / sqrt(len2(d')) with
 *               len2(d') = (d'.x*d'.x + d'.y*d'.y) + d'.z*d'.z.  Metal and dielectric vertices take no
 *               sample, so the next hit's ws is 1.
 *   continue    att = att * a (per channel); the next ray is the scatter's; the next segment's draws follow the
 *               light sample's.
 * The sample's value is rad.  Only + - * /, a correctly rounded sqrt, comparisons and selects, in the order
 * written (no fused multiply-add).
 * Why it is unbiased: the Lambertian scatter has solid-angle density cx / pi, which is gs in area measure at the
 * light; the light sample's area density is pl; the weights are the balance heuristic (the ws = 0 form hands the
 * whole contribution to the light sample).  The expectation equals rt_render's at the same max_depth, up to the
 * shadow interval's 2^-20 gap; unlisted emitters and the sky are never re-weighted.  With RT_NEE_MIS every
 * light term is bounded by a * Le, so area sampling's 1 / distance^4 outliers are gone.
 * RT_E_INVALID: unknown flag bits, tile_world != 1, a bad sample range, a NULL output.  Scenes with book-2
 * objects return RT_E_UNSUPPORTED.  rt_render_nee blocks; rt_render_nee_device takes a device pointer and is
 * asynchronous on `stream` (NULL: the context's stream). */
enum { RT_NEE_MIS = 1 }; /* flags */
int rt_render_nee(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params, int32_t flags,
                  double* accum_host /* [H][W][3] */);
int rt_render_nee_device(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params, int32_t flags,
                         double* accum_dev, void* stream);

/* ---- the adaptive light-sampling render --------------------------------------------
 * Added within ABI 11 like the light list: purely additive, RT_ABI_VERSION stays 11.
 *
 * rt_render_nee_adaptive is rt_render_adaptive's contract with rt_render_nee's samples, rendered by one kernel
 * launch: the wave that owns an 8x8 tile keeps the tile's statistics and takes the stop decision itself.
 * `flags` means what it means for rt_render_nee; the scene's light pick, light sampling mode and light
 * visibility settings apply as they do there.  params / adaptive are checked as for rt_render_adaptive: the batch
 * b = params->sample_chunk (0 means 4); params->samples (the per-pixel maximum), min_samples and step are
 * multiples of b; min_samples >= 2 b; sample_begin and sample_count are 0 and tile_world is 1.  engine and
 * scratch_mb are ignored.
 *
 *   samples     Sample s of pixel p is rt_render_nee's sample (seed, p, s).  The batch sum B_k(p) is the in-order
 *               sum of samples [k b, (k + 1) b) of p from (0, 0, 0): what rt_render_nee returns for that sample
 *               range, bit for bit.
 *   sums        A pixel that received n batches holds accum_c = ((0 + B_0.c) + B_1.c) + ... + B_(n-1).c per
 *               channel c, and, with y_k = (B_k.r + B_k.g) + B_k.b, the moments
 *               m1 = ((0 + y_0) + y_1) + ... + y_(n-1);  m2 = fma(y_k, y_k, m2) for k = 0 ... n-1 from m2 = 0
 *               (one rounding per batch) — rt_render_adaptive's sums, with rt_render_nee's batch sums.
 *   checks      A tile is checked when all its in-image pixels hold N = min_samples samples, then after every
 *               further `step`, the last one clipped at params->samples.  At a check after n = N / b batches:
 *                 v_p = max(0, m2_p - m1_p * m1_p / (double)n) / (double)(n - 1)  per in-image pixel p;
 *                 E = sum v_p, M = sum m1_p, K = the number of in-image pixels, each summed over the tile's 64
 *                 lanes (lane l = pixel (l % 8, l / 8) of the tile, out-of-image lanes contributing 0) by six
 *                 rounds off = 32, 16, 8, 4, 2, 1 in which every lane l adds lane (l ^ off)'s value to its own;
 *                 e = 0 if E == 0, else sqrt((double)n * E / K) / (M / K + ((double)n * b) * noise_floor).
 *               The tile goes on iff (!(e <= threshold) || threshold == 0) and N < params->samples.
 *   outputs     counts = N at the tile's last check, for every in-image pixel of the tile; tile_error = e at that
 *               check.  Threshold 0 stops no tile; +inf stops every tile with a finite e at min_samples; a NaN
 *               e renders to params->samples.
 * max_depth <= 0 gives zero sums, zero moments, counts = min_samples and e = 0; no segment is traced.
 * Every in-image element of every output is written by the call.  The result does not depend on which wave
 * renders which tile or on the size of the grid.
 *
 * rt_render_nee_adaptive blocks.  report (may be NULL): steps = 1 + ceil((largest count - min_samples) / step);
 * tiles = the tiles of the frame; tiles_converged = the tiles with e <= threshold at their last check (at
 * threshold 0 that counts the tiles with e == 0, all-sky tiles for one, although threshold 0 stopped none of them);
 * samples = the sum of counts; kernel_ms = the launch's event time; segments = 0 (this pass does not count
 * segments) and fold_ms = 0 (there is no fold).  rt_render_nee_adaptive_device takes device pointers (accum,
 * counts and moments required) and is asynchronous on `stream` (NULL: the context's stream) with no host
 * synchronisation; the tile counter is one word of the context, so at most one such call per context may be in
 * flight: issue the next on the same stream, or after the earlier one has completed.  rt_moments_variance,
 * rt_tonemap_counts and rt_denoise take the outputs as they take rt_render_adaptive's.  RT_E_INVALID: a failed check of params / adaptive, unknown flag bits, a NULL required
 * buffer.  Scenes with book-2 objects return RT_E_UNSUPPORTED.  Not available through the multi-GPU entry points;
 * not checkpointed. */
int rt_render_nee_adaptive(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params, int32_t flags,
                           const rt_adaptive_params* adaptive,
                           double* accum_host,      /* [H][W][3] sums over each pixel's own samples, row 0 = bottom */
                           int32_t* counts_host,    /* [H][W] samples the pixel received */
                           double* moments_host,    /* [H][W][2] m1, m2; may be NULL */
                           double* tile_error_host, /* [tiles] as rt_render_adaptive's; may be NULL */
                           rt_adaptive_report* report /* may be NULL */);
int rt_render_nee_adaptive_device(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* params, int32_t flags,
                                  const rt_adaptive_params* adaptive, double* accum_dev, int32_t* counts_dev,
                                  double* moments_dev, double* tile_error_dev /* may be NULL */, void* stream);

/* ---- the spatially weighted light pick ---------------------------------------------
 * Added within ABI 11 like the light list: purely additive, RT_ABI_VERSION stays 11.
 *
 * A scene-level setting that rt_render_direct and rt_render_nee (host and _device forms) read: with it the one
 * light per vertex is picked, on the same draw D, from a table row that depends on where the vertex lies, in
 * place of the uniform pick.  rt_scene_upload resets it to the uniform pick, so a caller that never sets it sees
 * no change.
 *
 * Light grid of a list of L >= 1 lights and `cells` in 1 ... 64.  IEEE binary64 throughout; only + - * /,
 * comparisons and selects, in the order written (no libm function, no fused multiply-add).
 *   box of light j   sphere: lo_a = c_a - r, hi_a = c_a + r, centre c;  rho2_j = r * r.
 *                    rect (d1, d2, axis as in rt_render_direct): h1 = (d1_max - d1_min) * 0.5,
 *                    h2 = (d2_max - d2_min) * 0.5; lo = (d1_min, d2_min, offset), hi = (d1_max, d2_max, offset),
 *                    centre = (d1_min + h1, d2_min + h2, offset) on (d1, d2, axis);  rho2_j = h1 * h1 + h2 * h2.
 *   grid box         lo_a = the least box lo_a, hi_a = the greatest box hi_a, taken in list order
 *                    (lo_a = b < lo_a ? b : lo_a; hi_a = b > hi_a ? b : hi_a, starting from light 0's).
 *   dimensions       ext_a = hi_a - lo_a;  ext_max = the greatest of ext_x, ext_y, ext_z (e > m ? e : m in this
 *                    order).  n_a = 1 if !(ext_a > 0); else f = (double)cells * (ext_a / ext_max) and
 *                    n_a = f < (double)cells ? 1 + (int)f : cells, which is min(cells, 1 + (int)f).
 *                    size_a = ext_a / (double)n_a.  A table of n_x * n_y * n_z * L > 2^22 entries is refused.
 *                    cells = 1 is one row: a position-independent, power-weighted pick.
 *   cell (ix,iy,iz)  row (iz * n_y + iy) * n_x + ix of L entries;  cell_lo_a = lo_a + (double)i_a * size_a,
 *                    cell_hi_a = lo_a + (double)(i_a + 1) * size_a.
 *   weights          s_j = (colour0 + colour1) + colour2;  Phi_j = area_j * (s_j > 0 ? s_j : 0)  (a NaN gives 0).
 *                    diag2 = (size_x * size_x + size_y * size_y) + size_z * size_z.
 *                    per axis t = cell_lo_a - c_a; t = t > 0 ? t : 0; e = c_a - cell_hi_a; d_a = e > t ? e : t.
 *                    D2 = (d_x * d_x + d_y * d_y) + d_z * d_z;  m = rho2_j + diag2;
 *                    w_j = Phi_j / (D2 > m ? D2 : m);  W = ((0 + w_0) + w_1) + ... in list order.
 *   row              if W > 0 and W < +inf:  p_j = ((w_j / W) * 0.875) + (0.125 / (double)L);
 *                    cdf_j = cdf_(j-1) + p_j from cdf_(-1) = 0, in list order.
 *                    otherwise (W is 0, +inf or a NaN):  cdf_j = (double)(j + 1) / (double)L.
 *                    Then cdf_(L-1) = 1.0 exactly.
 *   The evenly spread eighth keeps every p_j >= 0.125 / L > 0, whatever the colours (0, negative, inf, NaN), and
 *   bounds every estimate at 8 times the uniform pick's.
 * Pick at a vertex x (a device function of its own, csrc/rt/light_pick.h):
 *   cell        per axis inv_a = n_a == 1 ? 0 : (double)n_a / (hi_a - lo_a);  q = (x_a - lo_a) * inv_a;
 *               i_a = !(q >= 0) ? 0 : q >= (double)n_a ? n_a - 1 : (int)q  (a NaN gives 0; a vertex outside the
 *               box takes the border cell: every row is a distribution over all L lights, so this is unbiased).
 *   light       xi0 = draw D;  k = the smallest index with xi0 < cdf_k in the cell's row (a lower-bound binary
 *               search whose trip count depends on L alone; L - 1 if there is none: xi0 >= 1 or a NaN).
 *   probability p = cdf_k - (k ? cdf_(k-1) : 0.0): up to rounding, the probability with which the search returns k.
 * rt_render_direct and rt_render_nee with the grid pick: everything as defined above, except
 *   pick        the light is k above, and pl = p / area in place of 1 / (area * (double)L):
 *   value       RT_NEE_MIS clear (and rt_render_direct): g = ((cx * cy) / d2) * ((area / p) / pi);
 *               RT_NEE_MIS set: gs = ((cx * cy) / d2) / pi;  pl = p / area;  g = gs / (pl + gs).
 *   emission    (rt_render_nee, RT_NEE_MIS set) the weight of a listed hit on light j uses
 *               pl = p_j(cell_prev) / area_j, p_j(c) = cdf_j - (j ? cdf_(j-1) : 0.0) in row c, where cell_prev is
 *               the cell of the vertex that took the light sample.
 *   With L = 1 every row is {1.0}, p = 1.0, and the frames equal the uniform pick's bit for bit.
 * Unbiased because every p_j > 0 in every row, the pick's probability is the p the estimator divides by, and the
 * row used depends on the vertex alone. */
typedef struct rt_light_grid {
  int32_t n[3];     /* cells along x, y, z (all 0 when n_lights == 0) */
  int32_t n_lights; /* L */
  double lo[3];     /* the grid's box */
  double hi[3];
} rt_light_grid;
/* The grid of a description's light list, without a device.  `info` (not NULL) receives the dimensions and the
 * box; cdf (may be NULL) has room for n[0] * n[1] * n[2] * n_lights doubles and receives the rows.  A scene
 * without a listed light: RT_OK, info all zero, nothing written to cdf.  RT_E_INVALID: a NULL or invalid scene,
 * cells outside 1 ... 64, a table of more than 2^22 entries. */
int rt_light_grid_host(const rt_scene_desc* scene, int32_t cells, rt_light_grid* info, double* cdf);
/* Sets the light pick of the uploaded scene.  cells = 0: the uniform pick.  cells in 1 ... 64: builds the grid of
 * the scene's light list, uploads it, and makes rt_render_direct / rt_render_nee use it until the next
 * rt_scene_upload or rt_scene_light_pick.  `info` (may be NULL) receives what rt_light_grid_host would report
 * (all zero for cells = 0).  A scene without a listed light: RT_OK; nothing is ever picked.  RT_E_INVALID: no
 * uploaded scene, cells < 0 or > 64, a table of more than 2^22 entries (the setting is then left as it was).
 * Blocks until work queued on the context's stream has finished, since it replaces what that work reads. */
int rt_scene_light_pick(rt_ctx* ctx, int32_t cells, rt_light_grid* info);
/* Runs only the pick, on the device, for n points (points [n][3], xi [n]) in the grid last set by
 * rt_scene_light_pick: light[i] = k and prob[i] = p for the vertex points[i] and the draw xi[i].  A test entry
 * point like rt_probe_segment.  RT_E_INVALID: no uploaded scene, the uniform pick is set, the scene lists no
 * light, n < 0, a NULL buffer with n > 0.  Blocks. */
int rt_light_pick_at(rt_ctx* ctx, int32_t n, const double* points, const double* xi, int32_t* light, double* prob);

/* ---- solid-angle sampling of sphere lights -----------------------------------------
 * Added within ABI 11 like the light list: purely additive, RT_ABI_VERSION stays 11.
 *
 * A scene-level setting that rt_render_direct and rt_render_nee (host and _device forms) read, like
 * rt_scene_light_pick and independent of it (all four combinations of pick and mode are valid).  In mode
 * RT_LIGHT_SAMPLE_SOLID_ANGLE a sphere light's sample is a uniform direction of the cone the sphere subtends
 * from the vertex, so every sample lands on the cap the vertex sees and the estimator has no cy / d2 factor.
 * Rect lights are sampled as above in both of these modes; RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL (further below) samples
 * them by solid angle too.  rt_scene_upload resets the mode to RT_LIGHT_SAMPLE_AREA, so a caller that never sets it
 * sees no change.
 *
 * IEEE binary64 throughout; only + - * /, a correctly rounded sqrt, comparisons and selects, in the order
 * written (no fused multiply-add, no libm function).
 * Light sample of a sphere light with centre c and radius r > 0 at a vertex (x, n), after the pick's draw D:
 *   wc = c - x;  dc2 = (wc.x*wc.x + wc.y*wc.y) + wc.z*wc.z
 *   inside     !(dc2 > r*r): the sample contributes 0, consumes no further draw and traces no ray; it still
 *              counts as taken.
 *   dc = sqrt(dc2);  a = wc / dc (per component)
 *   s2 = (r*r) / dc2;  cm = sqrt(1.0 - s2);  om = s2 / (1.0 + cm)      (= 1 - cos(theta_max), no cancellation)
 *   basis      sg = a.z < 0 ? -1.0 : 1.0;  A = -1.0 / (sg + a.z);  B = (a.x * a.y) * A
 *              t1 = (1.0 + ((sg * a.x) * a.x) * A,  sg * B,  -(sg * a.x))
 *              t2 = (B,  sg + (a.y * a.y) * A,  -a.y)                   (|sg + a.z| >= 1 always)
 *   disk       (px, py) = random_in_unit_disk on draws D+1, ... (two per attempt, each -1 + 2 * draw, accepted
 *              when px*px + py*py <= 1: the camera lens's function)
 *   q = px*px + py*py;  e = q * om;  ct = 1.0 - e;  k = sqrt(om * (1.0 + ct))
 *              (q is uniform on [0, 1] and independent of the disk point's angle, so no sin / cos is needed:
 *              ct = cos(theta) is uniform on [1 - om, 1], and (px, py) * k = sin(theta) * (cos(phi), sin(phi)))
 *   omega = (t1 * (px * k) + t2 * (py * k)) + a * ct                    (per component, in this order)
 *   st2 = e * (1.0 + ct);  disc = r*r - dc2 * st2;  disc = disc > 0 ? disc : 0
 *   ds = dc * ct - sqrt(disc);  w = omega * ds
 *   u = ((x + w) - c) / r (per component)
 *   then as in rt_render_direct: d2 = len2(w); dist = sqrt(d2); cx = dot(n, w) / dist; cy = -dot(u, w) / dist;
 *              the cut !(cx > 0 && cy > 0); the shadow ray (x, w) on [0.001, 1 - 2^-20]; Le (FairyLight:
 *              colour * cy).
 *   value      RT_NEE_MIS clear and rt_render_direct:
 *                g = cx * ((2.0 * om) * (double)L)           grid pick: g = cx * ((2.0 * om) / p)
 *              RT_NEE_MIS set:
 *                gs = cx / pi;  pl = 1.0 / (((2.0 * pi) * om) * (double)L)      grid pick: pl = p / ((2.0 * pi) * om)
 *                g = gs / (pl + gs)
 *              value_c = (a_c * Le_c) * g
 * Emission weight (rt_render_nee): when the hit is a listed sphere, front_face holds and the previous vertex took
 * a sample, with o the origin of the segment's ray (the previous vertex): wc = c - o, dc2, s2, cm, om as above;
 *   !(dc2 > r*r) or !(cx_prev > 0):  ws = 1;
 *   else RT_NEE_MIS set:    gs = cx_prev / pi;  pl as above, with p_j(cell_prev) under the grid pick;
 *                           ws = gs / (pl + gs);
 *   else RT_NEE_MIS clear:  ws = 0.
 * Rect hits and everything else keep rt_render_nee's text.
 * Why it is unbiased: the cone's solid angle is 2 pi om, so the light sample's solid-angle density is
 * 1 / (2 pi om) per pick (times 1 / L or p for the pick) over exactly the directions that meet the sphere; the
 * plain estimator is f cos / density = (a / pi) Le cx (2 pi om) / pick.  The Lambertian scatter's density is cx / pi per solid angle, and the weights are the balance heuristic
 * in that measure at the previous vertex — the measure changes, the two densities' ratio does not.  From inside a
 * sphere both modes give the light sample nothing (area: cy <= 0 everywhere), and the scatter keeps the emission
 * whole. */
enum { RT_LIGHT_SAMPLE_AREA = 0, RT_LIGHT_SAMPLE_SOLID_ANGLE = 1 };

/* ---- solid-angle sampling of rect lights -------------------------------------------
 * Added within ABI 11 like the light list: purely additive, RT_ABI_VERSION stays 11.
 *
 * A third mode of the same setting.  RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL samples sphere lights exactly as
 * RT_LIGHT_SAMPLE_SOLID_ANGLE does, and a rect light by a uniform direction of the spherical rectangle it subtends
 * from the vertex (Urena, Fajardo and King 2013, "An area-preserving parametrization for spherical rectangles"), so
 * the rect's estimator has no cy / d2 factor either.  Modes 0 and 1 keep every bit of their behaviour.  "Rects only"
 * is not offered: the value 2 is not a mode and stays RT_E_INVALID, like every other value.
 *
 * IEEE binary64 throughout; + - * /, a correctly rounded sqrt, comparisons and selects, in the order written (no
 * fused multiply-add), and three functions sin, cos and acos that are NOT a libm's: they are pl_sin, pl_acos
 * (csrc/rt/portable_libm.h; pl_acos through pl_atan2) and pl_cos (csrc/rt/portable_trig.h: pl_sin's reduction and
 * its two polynomial kernels, in the cosine's quadrant order), each a fixed sequence of such operations and rint
 * (round to nearest, ties to even), so a restatement gives the same bits.  pi = 3.141592653589793,
 * twopi = 6.283185307179586.
 * Light sample of a listed rect at a vertex (x, n), after the pick's draw D.  (d1, d2, axis) are the rect's two
 * in-plane axes and its normal axis as in rt_render_direct; the rect is axis-aligned, so the local frame is this
 * permutation of the coordinates and nothing is normalised.
 *   x0 = d1_min - x[d1];  x1 = d1_max - x[d1];  y0 = d2_min - x[d2];  y1 = d2_max - x[d2];  z0 = offset - x[axis]
 *   coplanar   z0 == 0: the sample contributes 0, consumes no further draw and traces no ray; it still counts as
 *              taken.
 *   flip       if z0 > 0: z0 = -z0, and w[axis] below is -z0 in place of z0.
 *   zz = z0*z0
 *   b0 = -y0 / sqrt(zz + y0*y0);  n1z = x1 / sqrt(zz + x1*x1);  b1 = y1 / sqrt(zz + y1*y1);
 *   n3z = -x0 / sqrt(zz + x0*x0)                      (the z components of the four side planes' unit normals)
 *   g0 = acos(-(b0 * n1z));  g1 = acos(-(n1z * b1));  g2 = acos(-(b1 * n3z));  g3 = acos(-(n3z * b0))
 *   k = (twopi - g2) - g3;  S = (g0 + g1) - k                               (S: the rect's solid angle)
 *   u = draw D+1;  v = draw D+2   (two draws exactly, as for the area form, whichever of the two cases follows)
 *   small      !(S >= 2^-20) (a NaN too): the sample is the AREA form's on u and v, with rt_render_direct's /
 *              rt_render_nee's own value text (y[d1] = d1_min + u * (d1_max - d1_min), ...; w = y - x).  The four
 *              acos carry an absolute error of order 2^-50, so above the bound S is good to about 2^-30 relative,
 *              a bias far below any frame's noise; below it the rect is so small in the vertex's sky that the
 *              area form has no tail to remove.
 *   otherwise  au = u * S + k
 *              fu = (cos(au) * b0 - b1) / sin(au)
 *              cu = 1.0 / sqrt(fu*fu + b0*b0);  cu = fu > 0 ? cu : -cu;  cu = cu < -1 ? -1 : cu > 1 ? 1 : cu
 *              xu = -(cu * z0) / sqrt(1.0 - cu*cu);  xu = xu < x0 ? x0 : xu > x1 ? x1 : xu
 *              dd = xu*xu + z0*z0;  d = sqrt(dd)
 *              h0 = y0 / sqrt(dd + y0*y0);  h1 = y1 / sqrt(dd + y1*y1);  hv = h0 + v * (h1 - h0);  hv2 = hv*hv
 *              yv = hv2 < 1.0 - 2^-40 ? (hv * d) / sqrt(1.0 - hv2) : y1
 *              w[d1] = xu;  w[d2] = yv;  w[axis] = z0 (flip: -z0)
 *   then as in rt_render_direct: d2 = len2(w); dist = sqrt(d2); cx = dot(n, w) / dist; cy = |w[axis]| / dist; the cut
 *              !(cx > 0 && cy > 0) (a NaN from a degenerate division above is cut); the shadow ray (x, w) on
 *              [0.001, 1 - 2^-20]; Le (FairyLight: colour * cy).
 *   value      (not `small`)  RT_NEE_MIS clear and rt_render_direct:
 *                g = cx * ((S * (double)L) / pi)                  grid pick: g = cx * ((S / p) / pi)
 *              RT_NEE_MIS set:
 *                gs = cx / pi;  pl = 1.0 / (S * (double)L)        grid pick: pl = p / S
 *                g = gs / (pl + gs)
 *              value_c = (a_c * Le_c) * g
 * Emission weight (rt_render_nee): when the hit is a listed rect and the previous vertex took a sample, with o the
 * origin of the segment's ray (the previous vertex): x0 ... S as above with o for x;
 *   z0 == 0 or !(cx_prev > 0):  ws = 1;
 *   else !(S >= 2^-20):     rt_render_nee's area-measure weight, unchanged (the light sample at o applied the same
 *                           rule at the same point, so the two densities stay a consistent pair);
 *   else RT_NEE_MIS set:    gs = cx_prev / pi;  pl as above, with p_j(cell_prev) under the grid pick;
 *                           ws = gs / (pl + gs);
 *   else RT_NEE_MIS clear:  ws = 0.
 * Sphere lights and sphere hits keep the text above; everything else keeps rt_render_nee's.
 * Why it is unbiased: (u, v) -> direction is area-preserving from the unit square times S onto the spherical
 * rectangle, so the light sample's solid-angle density is 1 / S per pick (times 1 / L or p for the pick) over
 * exactly the directions that meet the rect; the plain estimator is f cos / density = (a / pi) Le cx S / pick.  The
 * Lambertian scatter's density is cx / pi per solid angle, and the weights are the balance heuristic in that
 * measure at the previous vertex, as for the cone.  A coplanar vertex sees the rect edge-on (cy = 0 for every
 * point of it), so nothing is lost there, and a scatter from it cannot hit the rect's face. */
enum { RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL = 3 };
/* Sets how rt_render_direct / rt_render_nee sample the uploaded scene's lights until the next rt_scene_upload or
 * rt_scene_light_sampling: RT_LIGHT_SAMPLE_AREA, RT_LIGHT_SAMPLE_SOLID_ANGLE (spheres) or
 * RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL (spheres and rects).  RT_E_INVALID: no uploaded scene, an unknown mode (the setting
 * is then left as it was).  Blocks until work queued on the context's stream has finished. */
int rt_scene_light_sampling(rt_ctx* ctx, int32_t mode);
/* Test entry points like rt_light_pick_at: vertex i = (points[i], normals[i]) runs the whole light sample except
 * the shadow ray, on the path key (seed, pixel = i, sample = 0) from draw 0, with a = 1 and no emitter scaling.
 *   light     the light picked;  draws: the path's draw counter after the sample.
 *   flags     1: cut, !(cx > 0 && cy > 0);  2: inside (a sphere by solid angle);  4: coplanar (a rect by solid
 *             angle).  g_plain = g_mis = 0 with any of them; inside and coplanar also leave w, cx and cy 0.
 *             8: small (a rect by solid angle whose sample is the area form's): a bit of its own that zeroes
 *             nothing and may come with 1.
 *   g_plain   g with RT_NEE_MIS clear;  g_mis: g with it set.
 * rt_light_sample_at runs on the device under the scene's current pick and mode.  rt_light_sample_host is plain
 * C++ without a device, compiled without contraction, and takes the pick (cells: 0 uniform, 1 ... 64 the grid)
 * and the mode as arguments.  RT_E_INVALID: no uploaded scene / a NULL or invalid scene, no listed light, n < 0, a
 * NULL buffer with n > 0, cells or mode out of range, a table of more than 2^22 entries.  n == 0 is RT_OK.
 * rt_light_sample_at blocks. */
typedef struct rt_light_sample {
  int32_t light;
  int32_t flags;
  uint32_t draws;
  int32_t pad;
  double w[3];
  double cx, cy;
  double g_plain, g_mis;
} rt_light_sample;
int rt_light_sample_at(rt_ctx* ctx, int32_t n, const double* points, const double* normals, uint64_t seed,
                       rt_light_sample* out);
int rt_light_sample_host(const rt_scene_desc* scene, int32_t cells, int32_t mode, int32_t n, const double* points,
                         const double* normals, uint64_t seed, rt_light_sample* out);

/* ---- visibility-aware light pick: traced occlusion per cell -------------------------
 * Added within ABI 11 like the light list: purely additive, RT_ABI_VERSION stays 11.
 *
 * A third scene-level setting, next to rt_scene_light_pick and rt_scene_light_sampling and independent of the
 * sampling mode.  It traces K shadow rays from every cell of the grid last set by rt_scene_light_pick to every
 * listed light and rebuilds every row with each light's weight multiplied by a smoothed share of the cell's points
 * that see the light.  rt_render_direct, rt_render_nee and rt_light_pick_at read other numbers in the rows and
 * nothing else.  rt_scene_upload and rt_scene_light_pick (any value) switch it off, so a caller that never sets it
 * sees no change.
 *
 * IEEE binary64 throughout; only + - * /, a correctly rounded sqrt, comparisons and selects, in the order written
 * (no fused multiply-add, no libm function).  rng(seed, pixel, sample, draw) is the counter RNG's draw: the
 * device's rng_next on Rng{pixel, sample, draw}.  The grid, lo, size_a, cell_lo_a, w_j, the row rule (above) and
 * the light record (rt_scene_lights) are as defined there.  Rays per pair: K in {1, 2, 4, 8, 16, 32}.
 * For cell row c = (iz * n_y + iy) * n_x + ix, cell point i in [0, K), light j in [0, L):
 *   cell point  x_a = cell_lo_a + rng(seed, c, i, a) * size_a for a = 0, 1, 2: shared by all lights of the cell.
 *   target      rect: xi1 = rng(seed, c, i, 4 + 2j), xi2 = rng(seed, c, i, 5 + 2j); y by rt_render_direct's `rect`
 *               rule (y[d1] = d1_min + xi1 * (d1_max - d1_min), y[d2] = d2_min + xi2 * (d2_max - d2_min),
 *               y[axis] = offset).  The draws start at an even index; draw 3 is unused.
 *               sphere (centre q, radius r): e = x - q;  e2 = (e.x*e.x + e.y*e.y) + e.z*e.z.
 *               !(e2 > r*r): the pair's bit i is set and no ray is traced.  Otherwise le = sqrt(e2) and
 *               y_a = q_a + r * (e_a / le): the light's nearest point, which is deterministic (the cone mode samples
 *               that cap anyway).
 *   ray         w = y - x;  w2 = (w.x*w.x + w.y*w.y) + w.z*w.z.  !(w2 > 0): the bit is set and no ray is traced.
 *               Otherwise the bit is set iff (x, w) is not occluded on [0.001, 1 - 2^-20] in the sense of
 *               rt_scene_occluded: the passes' shadow interval.
 *   mask        mask[c][j] is a uint32 whose bit i is the above.
 *   rows        per cell: valid = mask[c][0] | mask[c][1] | ...;  Kc = popcount(valid).  A point that no light sees
 *               is dead: it lies inside an object, and every light's count skips it.
 *               Kc == 0: the cell keeps rt_scene_light_pick's row.
 *               otherwise u_j = popcount(mask[c][j]);  v_j = ((double)u_j + 1.0) / ((double)Kc + 2.0);
 *               w'_j = w_j * v_j;  W' = ((0 + w'_0) + w'_1) + ... in list order; then the `row` rule above with w',
 *               W' in place of w, W: the 0.875 / 0.125 split, the fallback for W' of 0, +inf or a NaN, and
 *               cdf_(L-1) = 1.0 exactly.  (Bits of a mask at or above K are ignored.)
 * Why it stays unbiased: every p_j >= 0.125 / L still; the table is fixed before any sample is drawn; the row
 * depends on the vertex's cell alone; and the estimator and the MIS weights divide by the p of the same rows, which
 * light_prob reads.  The bound "8 times the uniform pick's" on every estimate still holds.  A wrong mask costs
 * variance, never expectation. */
typedef struct rt_light_visibility {
  int32_t rays, pad;    /* K; 0 when off */
  uint64_t seed;
  uint64_t pairs;       /* cells * L */
  uint64_t traced;      /* shadow rays traced (bits decided without a ray are not counted) */
  uint64_t unoccluded;  /* bits set */
  uint64_t dead_points; /* cell points no light sees */
  double kernel_ms;     /* device time of the trace kernel */
} rt_light_visibility;
/* Traces the masks of the uploaded scene in the grid last set by rt_scene_light_pick, builds the rows on the host
 * and uploads them in place of the grid's, until the next rt_scene_upload, rt_scene_light_pick or
 * rt_scene_light_visibility.  rays = 0 puts rt_scene_light_pick's rows back (RT_OK too when nothing was set).
 * `report` (may be NULL) receives the counts (all zero for rays = 0).  RT_E_INVALID: no uploaded scene, rays not 0,
 * 1, 2, 4, 8, 16 or 32, the uniform pick is set, the scene lists no light (the setting is then left as it was).
 * RT_E_UNSUPPORTED: a scene with book-2 objects, like rt_scene_occluded.  Blocks, like rt_scene_light_pick. */
int rt_scene_light_visibility(rt_ctx* ctx, int32_t rays, uint64_t seed, rt_light_visibility* report);
/* Test entry point: the masks the device traced for the setting in force, [cells][L].  RT_E_INVALID: no uploaded
 * scene, the setting is off, a NULL buffer. */
int rt_light_visibility_masks(rt_ctx* ctx, uint32_t* masks);
/* The K rays of one (cell, light) pair, without a device: rays_out [K][6] = x, w and traced [K] = 1 where the ray
 * is traced, 0 where the bit is set without one (w is 0, 0, 0 from inside a sphere light).  RT_E_INVALID: a NULL
 * or invalid scene, a NULL buffer, cells outside 1 ... 64, a table of more than 2^22 entries, rays not one of the six
 * values, no listed light, cell or light out of range. */
int rt_light_visibility_rays_host(const rt_scene_desc* scene, int32_t cells, int32_t rays, uint64_t seed, int32_t cell,
                                  int32_t light, double* rays_out, uint8_t* traced);
/* The rows for given masks ([cells][L]), without a device: cdf as rt_light_grid_host lays it out.  RT_E_INVALID: as
 * above (no cell, light or seed here). */
int rt_light_visibility_rows_host(const rt_scene_desc* scene, int32_t cells, int32_t rays, const uint32_t* masks,
                                  double* cdf);

#ifdef __cplusplus
}
#endif
#endif /* SHIRLEY_RT_H */
