// rt_multi.cpp — the multi-GPU entry points of the C ABI (include/shirley_rt.h): RCCL communicators,
// rt_render_sharded (one process per GPU) and rt_render_multi (one process driving several GPUs).
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_ctx.h"

using namespace rt;

namespace {

#define RCCL_TRY(ctx, expr)                                                                       \
  do {                                                                                            \
    ncclResult_t r_ = (expr);                                                                     \
    if (r_ != ncclSuccess) return fail(ctx, RT_E_RCCL, "%s: %s (%s:%d)", #expr, rccl().GetErrorString(r_), \
                                       __FILE__, __LINE__);                                       \
  } while (0)

int need_rccl(rt_ctx* c) {
  if (!rccl().ok()) return fail(c, RT_E_RCCL, "%s", rccl().error.c_str());
  return RT_OK;
}

// Partition of a multi-GPU frame (rt_render_params.partition): RT_PARTITION_AUTO picks the measured
// default; SHIRLEY_PARTITION=tiles|samples overrides it (tuning).
int frame_partition(rt_ctx* c, const rt_render_params* p, int world, int* out) {
  int part = p->partition;
  if (part < RT_PARTITION_AUTO || part > RT_PARTITION_SAMPLES) return fail(c, RT_E_INVALID, "bad partition %d", part);
  if (part == RT_PARTITION_AUTO) {
    part = RT_PARTITION_TILES;
    if (const char* e = getenv("SHIRLEY_PARTITION")) part = !strcmp(e, "samples") ? RT_PARTITION_SAMPLES : RT_PARTITION_TILES;
  }
  (void)world;
  *out = part;
  return RT_OK;
}

// Row bands of a sample-partitioned frame: rank b owns rows [b * band_rows, (b + 1) * band_rows).
int band_rows(const rt_camera* cam, int world) { return (cam->image_height + world - 1) / world; }

// One rank's share before the exchange.
//   tiles: its tiles rendered into c->packed ([max_tiles][64][3]); *count = doubles per rank of the gather
//     (rank 0 also sizes the gathered buffer).
//   samples: all pixels for its part of the frame's sample range, rendered into c->packed as
//     [world * band_rows][W][3] (rows >= H zero); *count = doubles of one row band.
int shard_render(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int part, int world, int rank,
                 hipStream_t s, size_t* count) {
  int st = check_render_args(c, cam, p);
  if (st) return st;
  HIP_TRY(c, hipSetDevice(c->device));
  SampleRange R;
  if ((st = resolve_range(c, p, &R))) return st;
  rt_render_params q = *p;
  q.tile_rank = 0;
  q.tile_world = 1;
  const int tiles_y = (cam->image_height + kTile - 1) / kTile;
  if (part == RT_PARTITION_SAMPLES) {
    const int rows = band_rows(cam, world);
    *count = (size_t)rows * cam->image_width * 3;
    const size_t total = *count * world;
    if ((st = ensure(c, c->packed, total * sizeof(double)))) return st;
    if ((st = ensure(c, c->parts, total * sizeof(double)))) return st;
    if ((st = ensure(c, c->band, *count * sizeof(double)))) return st;
    if (rank == 0 && (st = ensure(c, c->gathered, total * sizeof(double)))) return st;
    const size_t image = (size_t)cam->image_height * cam->image_width * 3;
    double* local = static_cast<double*>(c->packed.p);
    HIP_TRY(c, hipSetDevice(c->device));
    if (total > image) HIP_TRY(c, hipMemsetAsync(local + image, 0, (total - image) * sizeof(double), s));
    const long long n = R.end - R.begin;
    SampleRange mine;
    mine.begin = R.begin + (int)(n * rank / world);
    mine.end = R.begin + (int)(n * (rank + 1) / world);
    return render_window(c, cam, &q, mine, 0, tiles_y, 0, cam->image_height, 0, local, s);
  }
  int32_t n_total = 0, max_tiles = 0;
  if (rt_tile_layout(cam, world, &n_total, &max_tiles)) return fail(c, RT_E_INVALID, "bad tile layout");
  *count = (size_t)max_tiles * kTilePixels * 3;
  if ((st = ensure(c, c->packed, std::max<size_t>(*count, 1) * sizeof(double)))) return st;
  if (rank == 0 && (st = ensure(c, c->gathered, std::max<size_t>(*count * world, 1) * sizeof(double)))) return st;
  q.tile_rank = rank;
  q.tile_world = world;
  return render_window(c, cam, &q, R, 0, tiles_y, 0, cam->image_height, 1, static_cast<double*>(c->packed.p), s);
}

// samples partition, after the all-to-all (c->parts = [world][band] partial bands of this rank's rows):
// the rank-order sum of its band
int shard_band_sum(rt_ctx* c, int world, size_t count, hipStream_t s) {
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, launch_sum_parts(static_cast<const double*>(c->parts.p), world, (long long)count,
                              static_cast<double*>(c->band.p), s));
  return RT_OK;
}

// Root: the gathered buffer -> accum_dev [H][W][3] (tiles: scatter the packed tiles; samples: the
// gathered row bands are the image's rows in order, padding rows dropped).
int shard_unpack(rt_ctx* c, const rt_camera* cam, int part, int world, double* accum_dev, hipStream_t s) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (part == RT_PARTITION_SAMPLES) {
    const size_t bytes = (size_t)cam->image_height * cam->image_width * 3 * sizeof(double);
    HIP_TRY(c, hipMemcpyAsync(accum_dev, c->gathered.p, bytes, hipMemcpyDeviceToDevice, s));
    return RT_OK;
  }
  int32_t n_total = 0, max_tiles = 0;
  rt_tile_layout(cam, world, &n_total, &max_tiles);
  const int tiles_x = (cam->image_width + kTile - 1) / kTile;
  HIP_TRY(c, launch_unpack(static_cast<const double*>(c->gathered.p), world, max_tiles, n_total, tiles_x,
                           cam->image_width, cam->image_height, accum_dev, s));
  return RT_OK;
}

// What every rank of a sharded frame must agree on: the scene (its digest) and the arguments that decide
// the collectives' shapes and the frame's bits — the resolved partition, the resolved sample range, samples,
// seed, max_depth, sample_chunk and the camera (field by field, no padding hashed).  FNV-1a, 64 bits.
uint64_t call_key(const rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int part, const SampleRange& R) {
  Fnv1a f;
  f.val(c->digest);
  f.val(part);
  f.val(R.begin);
  f.val(R.end);
  f.val(p->samples);
  f.val(p->seed);
  f.val(p->max_depth);
  f.val(p->sample_chunk);
  f.val(cam->image_width);
  f.val(cam->image_height);
  f.val(cam->height);
  f.val(cam->width);
  f.val(cam->focal_length);
  f.val(cam->has_lens);
  f.val(cam->lens_radius);
  f.bytes(cam->origin, sizeof cam->origin);
  f.bytes(cam->w, sizeof cam->w);
  f.bytes(cam->u, sizeof cam->u);
  f.bytes(cam->v, sizeof cam->v);
  f.val(cam->focus_length);
  f.val(cam->time0);
  f.val(cam->time1);
  return f.h;
}

// The gathered words of one call: RT_OK, or RT_E_INVALID naming the first rank that differs from rank 0.
int key_verdict(rt_ctx* c, const uint64_t* words, int world) {
  int what = 0;
  const int r = key_mismatch(words, world, &what);
  if (r < 0) return RT_OK;
  if (what == 0)
    return fail(c, RT_E_INVALID, "scene mismatch across ranks: rank %d holds scene %016llx, rank 0 %016llx", r,
                (unsigned long long)words[2 * r], (unsigned long long)words[0]);
  return fail(c, RT_E_INVALID,
              "render arguments differ across ranks (partition, sample range, samples, seed, max_depth, "
              "sample_chunk or camera): rank %d key %016llx, rank 0 %016llx",
              r, (unsigned long long)words[2 * r + 1], (unsigned long long)words[1]);
}

// Every rank must render the same scene with the same call key (keycheck.h states the rule).  Every call
// all-gathers each rank's 16-byte (scene digest, key) on every rank — one collective sequence on all ranks
// whatever their arguments — copies the gathered words into pinned host memory and checks them: at once
// when this rank's key is new (or SHIRLEY_KEY_CHECK=sync), else at the next call (no host round trip in a
// steady loop of frames).  A failed check leaves no frame collective issued by this rank.
int check_call_key(rt_ctx* c, rt_comm* m, uint64_t key, hipStream_t s) {
  const int W = m->world;
  const size_t slot_words = 2 * (size_t)(W + 1);
  int st;
  if (!m->key_words) {
    HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&m->key_words), 2 * slot_words * sizeof(uint64_t), 0));
    for (hipEvent_t& e : m->key_ev) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  // the previous call's words: the deferred half of its check
  if (m->ks.pending) {
    m->ks.pending = false;
    HIP_TRY(c, hipEventSynchronize(m->key_ev[m->key_pending]));
    if ((st = key_verdict(c, m->key_words + m->key_pending * slot_words, W))) {
      m->ks.verified = false;
      m->ks.poisoned = true;
      return st;
    }
  }
  if ((st = ensure(c, c->digests, 2 * slot_words * sizeof(uint64_t)))) return st;
  const int slot = m->key_slot;
  m->key_slot ^= 1;
  uint64_t* hw = m->key_words + slot * slot_words;  // (this slot's last check was done: at most one pending)
  uint64_t* dw = static_cast<uint64_t*>(c->digests.p) + slot * slot_words;
  hw[2 * W] = c->digest;
  hw[2 * W + 1] = key;
  HIP_TRY(c, hipMemcpyAsync(dw + 2 * W, hw + 2 * W, 2 * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  RCCL_TRY(c, rccl().AllGather(dw + 2 * W, dw, 2, ncclUint64, m->comm, s));
  HIP_TRY(c, hipMemcpyAsync(hw, dw, 2 * (size_t)W * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipEventRecord(m->key_ev[slot], s));
  const char* e = getenv("SHIRLEY_KEY_CHECK");
  if (key_check_now(m->ks, key, e && !strcmp(e, "sync"))) {
    HIP_TRY(c, hipEventSynchronize(m->key_ev[slot]));
    if ((st = key_verdict(c, hw, W))) {
      m->ks.verified = false;
      m->ks.poisoned = true;
      return st;
    }
    m->ks.verified = true;
    m->ks.verified_key = key;
  } else {
    m->ks.pending = true;
    m->key_pending = slot;
  }
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES]) {
  if (!id) return RT_E_INVALID;
  if (!rccl().ok()) return RT_E_RCCL;
  ncclUniqueId u;
  static_assert(sizeof u == RT_COMM_ID_BYTES, "ncclUniqueId size");
  if (rccl().GetUniqueId(&u) != ncclSuccess) return RT_E_RCCL;
  std::memcpy(id, &u, sizeof u);
  return RT_OK;
}

int rt_comm_init_rank(rt_ctx* c, const uint8_t id[RT_COMM_ID_BYTES], int32_t world, int32_t rank, rt_comm** out) {
  if (!c) return RT_E_INVALID;
  if (!id || !out || world < 1 || rank < 0 || rank >= world)
    return fail(c, RT_E_INVALID, "bad communicator arguments (world %d, rank %d)", world, rank);
  *out = nullptr;
  int st = need_rccl(c);
  if (st) return st;
  HIP_TRY(c, hipSetDevice(c->device));
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof u);
  rt_comm* m = new rt_comm();
  m->world = world;
  m->rank = rank;
  m->device = c->device;
  const ncclResult_t r = rccl().CommInitRank(&m->comm, world, u, rank);
  if (r != ncclSuccess) {
    delete m;
    return fail(c, RT_E_RCCL, "ncclCommInitRank(world %d, rank %d): %s", world, rank, rccl().GetErrorString(r));
  }
  *out = m;
  return RT_OK;
}

int rt_comm_destroy(rt_comm* m) {
  if (!m) return RT_OK;
  (void)hipSetDevice(m->device);
  if (m->comm && rccl().ok()) (void)rccl().CommDestroy(m->comm);
  for (hipEvent_t e : m->key_ev)
    if (e) (void)hipEventDestroy(e);
  if (m->key_words) (void)hipHostFree(m->key_words);
  delete m;
  return RT_OK;
}

int rt_render_sharded(rt_ctx* c, rt_comm* m, const rt_camera* cam, const rt_render_params* p, double* accum_dev,
                      void* stream) {
  if (!c) return RT_E_INVALID;
  if (!m || !m->comm) return fail(c, RT_E_INVALID, "no communicator");
  if (m->device != c->device) return fail(c, RT_E_INVALID, "communicator of device %d used with device %d", m->device, c->device);
  if (m->ks.poisoned)  // (keycheck.h: its peers may still hold the failed call's frame collectives)
    return fail(c, RT_E_INVALID, "communicator poisoned by a failed cross-rank check: destroy and re-create it");
  if (m->rank == 0 && !accum_dev) return fail(c, RT_E_INVALID, "accum_dev is NULL on the root");
  if (!c->have_scene) return fail(c, RT_E_INVALID, "no scene uploaded (call rt_scene_upload first)");
  if (!p || !cam) return fail(c, RT_E_INVALID, "camera/params is NULL");
  int part = 0;
  int st = frame_partition(c, p, m->world, &part);
  if (st) return st;
  if ((st = check_render_args(c, cam, p))) return st;
  SampleRange R;
  if ((st = resolve_range(c, p, &R))) return st;
  hipStream_t s;
  resolve_stream(c, stream, &s);
  HIP_TRY(c, hipSetDevice(c->device));
  if ((st = check_call_key(c, m, call_key(c, cam, p, part, R), s))) return st;
  size_t count = 0;
  if ((st = shard_render(c, cam, p, part, m->world, m->rank, s, &count))) return st;
  if (part == RT_PARTITION_SAMPLES) {
    RCCL_TRY(c, rccl().AllToAll(c->packed.p, c->parts.p, count, ncclFloat64, m->comm, s));
    if ((st = shard_band_sum(c, m->world, count, s))) return st;
    RCCL_TRY(c, rccl().Gather(c->band.p, m->rank == 0 ? c->gathered.p : nullptr, count, ncclFloat64, 0, m->comm, s));
  } else {
    RCCL_TRY(c, rccl().Gather(c->packed.p, m->rank == 0 ? c->gathered.p : nullptr, count, ncclFloat64, 0, m->comm, s));
  }
  if (m->rank == 0) return shard_unpack(c, cam, part, m->world, accum_dev, s);
  return RT_OK;
}

int rt_render_multi(rt_ctx* const* ctxs, int32_t n, const rt_camera* cam, const rt_render_params* p,
                    double* accum_host) {
  if (!ctxs || n < 1 || !ctxs[0]) return RT_E_INVALID;
  rt_ctx* root = ctxs[0];
  if (!cam || !p || !accum_host) return fail(root, RT_E_INVALID, "NULL argument");
  if (p->tile_world != 1) return fail(root, RT_E_INVALID, "rt_render_multi shards the frame itself (tile_world must be 1)");
  std::vector<int> devs(n);
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i]) return fail(root, RT_E_INVALID, "ctxs[%d] is NULL", i);
    devs[i] = ctxs[i]->device;
    for (int j = 0; j < i; ++j)
      if (devs[j] == devs[i]) return fail(root, RT_E_INVALID, "device %d appears twice", devs[i]);
  }
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i]->have_scene) return fail(root, RT_E_INVALID, "device %d: no scene uploaded", devs[i]);
    if (ctxs[i]->digest != root->digest)
      return fail(root, RT_E_INVALID, "scene mismatch: device %d holds scene %016llx, device %d %016llx", devs[i],
                  (unsigned long long)ctxs[i]->digest, devs[0], (unsigned long long)root->digest);
  }
  int part = 0;
  int st = frame_partition(root, p, n, &part);
  if (st) return st;
  if ((st = need_rccl(root))) return st;
  if (root->group_devices != devs) {  // (re)build the communicators of this device set
    for (rt_comm& m : root->group_comms)
      if (m.comm) (void)rccl().CommDestroy(m.comm);
    root->group_comms.clear();
    root->group_devices.clear();
    std::vector<ncclComm_t> comms(n, nullptr);
    RCCL_TRY(root, rccl().CommInitAll(comms.data(), n, devs.data()));
    for (int i = 0; i < n; ++i) root->group_comms.push_back(rt_comm{comms[i], n, i, devs[i]});
    root->group_devices = devs;
  }
  // every device renders its share (asynchronous, all devices at once), then grouped collectives
  std::vector<size_t> count(n);
  for (int i = 0; i < n; ++i) {
    if ((st = shard_render(ctxs[i], cam, p, part, n, i, ctxs[i]->stream, &count[i])))
      return i ? fail(root, st, "device %d: %s", devs[i], ctxs[i]->err.c_str()) : st;
  }
  auto grouped = [&](auto&& one) -> int {
    RCCL_TRY(root, rccl().GroupStart());
    for (int i = 0; i < n; ++i) {
      const ncclResult_t r = one(i);
      if (r != ncclSuccess) {
        (void)rccl().GroupEnd();
        return fail(root, RT_E_RCCL, "collective (rank %d): %s", i, rccl().GetErrorString(r));
      }
    }
    RCCL_TRY(root, rccl().GroupEnd());
    return RT_OK;
  };
  if (part == RT_PARTITION_SAMPLES) {
    if ((st = grouped([&](int i) {
           return rccl().AllToAll(ctxs[i]->packed.p, ctxs[i]->parts.p, count[i], ncclFloat64, root->group_comms[i].comm,
                                  ctxs[i]->stream);
         })))
      return st;
    for (int i = 0; i < n; ++i)
      if ((st = shard_band_sum(ctxs[i], n, count[i], ctxs[i]->stream))) return i ? fail(root, st, "device %d: %s", devs[i], ctxs[i]->err.c_str()) : st;
    if ((st = grouped([&](int i) {
           return rccl().Gather(ctxs[i]->band.p, i == 0 ? root->gathered.p : nullptr, count[i], ncclFloat64, 0,
                                root->group_comms[i].comm, ctxs[i]->stream);
         })))
      return st;
  } else {
    if ((st = grouped([&](int i) {
           return rccl().Gather(ctxs[i]->packed.p, i == 0 ? root->gathered.p : nullptr, count[i], ncclFloat64, 0,
                                root->group_comms[i].comm, ctxs[i]->stream);
         })))
      return st;
  }
  const size_t bytes = (size_t)cam->image_width * cam->image_height * 3 * sizeof(double);
  HIP_TRY(root, hipSetDevice(root->device));
  if ((st = ensure(root, root->accum, bytes))) return st;
  if ((st = shard_unpack(root, cam, part, n, static_cast<double*>(root->accum.p), root->stream))) return st;
  HIP_TRY(root, hipMemcpyAsync(accum_host, root->accum.p, bytes, hipMemcpyDeviceToHost, root->stream));
  for (int i = n - 1; i >= 0; --i) {
    HIP_TRY(root, hipSetDevice(ctxs[i]->device));
    HIP_TRY(root, hipStreamSynchronize(ctxs[i]->stream));
  }
  return RT_OK;
}

}  // extern "C"
