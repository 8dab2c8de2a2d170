// rt_launch.h — the launch wrappers of the HIP files, as the host side of the C ABI calls them.
//
// Included by rt_api.cpp, rt_multi.cpp, rt_denoise.cpp and by the files that define the wrappers (trace.hip,
// trace_split.hip, wavefront.hip, features.hip, denoise.hip, occlusion.hip, direct.hip, nee.hip, nee_adaptive.hip), so a changed
// signature fails to compile where it is changed.  The wrappers of the tile passes and of the ray batches
// (launch_features, _occluded, _ao, _direct, _nee, _hit4, _probe) keep their own argument checks and place and
// launch their kernel through pass_frame.h (dispatch_placement, block_lds_bytes, launch_block).
#pragma once

#include <hip/hip_runtime.h>

#include "rt_layout.h"

namespace rt {
struct DLightGrid;  // light_pick.h
// trace.hip
hipError_t trace_occupancy(const DScene& S, int threads, int hop, int* blocks_per_cu);
hipError_t launch_trace(const KParams& p, int blocks, int threads, int hop, hipStream_t stream);
#ifdef RT_PHASE_TIMING
void phase_counters_dump();
#endif
#ifdef RT_TIMELINE
void timeline_dump();
#endif
hipError_t launch_reduce(const double* partial, int n_chunks, int n_tiles_rank, int tiles_x, int ty0, int tile_rank,
                         int tile_world, int width, int row0, int row1, int packed, int accumulate, double* out,
                         hipStream_t stream);
hipError_t launch_fold_stats(const double* partial, int n_chunks, int n_list, const uint32_t* tile_list, int tiles_x,
                             int width, int height, long long n_batches, int batch, double noise_floor,
                             double* accum, double* moments, double* err, hipStream_t stream);
hipError_t launch_tonemap_counts(const double* accum, const int32_t* counts, int width, int height, uint8_t* rgb8,
                                 hipStream_t stream);
hipError_t launch_tonemap(const double* accum, int width, int height, double inv, uint8_t* rgb8, hipStream_t stream);
hipError_t launch_unpack(const double* gathered, int world, int max_tiles, int n_tiles_total, int tiles_x, int width,
                         int height, double* out, hipStream_t stream);
hipError_t launch_sum_parts(const double* parts, int n_parts, long long n, double* out, hipStream_t stream);
hipError_t launch_hit(const DScene& S, const double* rays, int n, double t_min, double t_max, void* out,
                      hipStream_t stream);
hipError_t launch_hit4(const DScene& S, bool wide, const double* rays, int n, double t_min, double t_max, void* out,
                       hipStream_t stream);
hipError_t launch_probe(const DScene& S, bool wide, const double* rays, int n, uint64_t seed, uint32_t sample,
                        uint32_t draw, void* out, hipStream_t stream);
// features.hip
hipError_t launch_features(const DScene& S, bool wide, const DCamera& C, uint64_t seed, int s_begin, int s_end,
                           int chain, double* albedo, double* normal, double* depth, hipStream_t stream);
// denoise.hip
hipError_t launch_denoise(const rt_denoise_inputs& in, const rt_denoise_params& prm, double* recs_a, double* recs_b,
                          double* out, hipStream_t stream);
hipError_t launch_moments_variance(const double* moments, const int32_t* counts, int batch, long long n, double* out,
                                   hipStream_t stream);
// occlusion.hip
hipError_t launch_occluded(const DScene& S, bool wide, bool closest, const double* rays, int n, double t_min,
                           double t_max, const double* t_max_each, uint8_t* out, hipStream_t stream);
hipError_t launch_ao(const DScene& S, bool wide, const DCamera& C, uint64_t seed, int s_begin, int s_end, int chain,
                     double radius, double* ao, hipStream_t stream);
// direct.hip
hipError_t launch_direct(const DScene& S, bool wide, const DCamera& C, uint64_t seed, int s_begin, int s_end, int chain,
                         const DLight* lights, int n_lights, const DLightGrid* grid, int sample, double* emission,
                         double* direct, hipStream_t stream);
hipError_t launch_light_pick(const DLightGrid& grid, int n_lights, int n, const double* points, const double* xi,
                             int32_t* light, double* prob, hipStream_t stream);
hipError_t launch_light_sample(const DLight* lights, int n_lights, const DLightGrid* grid, int sample, uint64_t seed,
                               int n, const double* points, const double* normals, rt_light_sample* out,
                               hipStream_t stream);
// nee.hip
hipError_t launch_nee(const DScene& S, bool wide, bool mis, const DCamera& C, uint64_t seed, int s_begin, int s_end,
                      int max_depth, const DLight* lights, int n_lights, const DLightGrid* grid, int sample,
                      const int32_t* prim_light, double* accum, hipStream_t stream);
// nee_adaptive.hip: the adaptive arguments of nee_kernel's ADAPT instances (rt_render_nee_adaptive)
struct NeeAdapt {
  unsigned* counter;  // the next tile to hand out: cleared on the stream before the launch
  double* moments;    // [H][W][2] m1, m2
  double* tile_err;   // [tiles] e at the tile's last check, or null
  int32_t* counts;    // [H][W]
  int batch, min_samples, step;
  double threshold, noise_floor;
};
hipError_t launch_nee_adaptive(const DScene& S, bool wide, bool mis, const DCamera& C, uint64_t seed, int samples,
                               int max_depth, const DLight* lights, int n_lights, const DLightGrid* grid, int sample,
                               const int32_t* prim_light, double* accum, const NeeAdapt& ad, int cu_count,
                               int max_blocks, hipStream_t stream);
// trace_split.hip
bool split_supported_nt(int nt);
hipError_t split_prepare(const DScene& S, int nt, int* blocks_per_cu);
hipError_t launch_split(const KParams& p, int nt, int blocks, hipStream_t stream);
// wavefront.hip
int wf_grid_threads();
hipError_t wf_prepare(const DScene& S, int* extend_blocks_per_cu);
hipError_t wf_prepare4(const DScene& S, int* extend_blocks_per_cu);
hipError_t wf_launch_extend4(const WfParams& P, int extend_blocks, hipStream_t s);
hipError_t wf_start(const WfParams& P, int grid_blocks, hipStream_t s);
hipError_t wf_launch_extend(const WfParams& P, int extend_blocks, hipStream_t s);
hipError_t wf_launch_shade(const WfParams& P, int grid_blocks, hipStream_t s);
hipError_t wf_launch_texture(const WfParams& P, int grid_blocks, hipStream_t s);
}  // namespace rt
