#!/usr/bin/env python3
"""Measurements of the visibility-aware light pick for DESIGN.md §21 (needs an MI355X; the product path only, no
oracle), by the protocol of tools/cone_measure.py:

  cost     night random, SAH tree, at (cells, K) in CONFIGS: the device time of the trace kernel (the report's
           kernel_ms) and the wall time of the whole rt_scene_light_visibility call, REPS times each after a warm-up
           call; next to it rt_scene_occluded_device over the same traced rays (rt_light_visibility_rays_host) in
           one batch, the host row build alone (rt_light_visibility_rows_host on the device's masks) and what is
           left of the call (the readback, the upload of the rows, the synchronisations).  And the device time of a
           16-spp rt_render_nee frame at 1200x800, the yardstick the call's cost is held against.
  payoff   night random 1200x800, RT_NEE_MIS set, against a REF_SPP-sample rt_render frame over samples
           [REF_BEGIN, REF_BEGIN + REF_SPP) (disjoint from every measured range): the error of the mean over samples
           [0, S), S in SPPS, of rt_render_nee with cone + 16 cells, the same + visibility K = 32, cone + 32 cells
           + visibility K = 16, and of rt_render at the sample count that fits each visibility row's time.
           Per-pixel error = RMS over the channels; recorded: its median, 99th percentile and maximum, the frame
           RMSE and the count of pixels off by more than 1.  Recorded, not asserted.
  lamps    the tests' lamp field with the added box at 32x32 (tests/test_gpu_light_visibility.py): the frame mean's
           standard error over 16 ranges of 16 spp with the plain grid's rows and with the visibility rows.

usage: tools/lightvis_measure.py OUT.json
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ((8, 8), (16, 32), (32, 16))
REPS = 3
PASSES = (("cone_cells16", 16, 0), ("cone_cells16_vis32", 16, 32), ("cone_cells32_vis16", 32, 16))


def log(row):
    print(json.dumps(row), file=sys.stderr, flush=True)


def _pair_chunk(job):
    """The traced rays of pairs [lo, hi), from the library's host function (a worker builds its own scene)."""
    cells, rays, seed, n_lights, lo, hi = job
    sys.path.insert(0, os.path.join(REPO, "shirley-raytracing-rs_amd"))
    import raytracer as rt
    sc = rt.scenes.random_scene(seed, night=True).finalize(seed)
    out, keep = np.zeros((hi - lo, rays, 6)), np.zeros((hi - lo, rays), dtype=bool)
    for pair in range(lo, hi):
        r, traced = rt.light_visibility_rays_host(sc, cells, rays, seed, pair // n_lights, pair % n_lights)
        out[pair - lo], keep[pair - lo] = r, traced == 1
    return out[keep]


def pair_rays(rt, sc, seed, workers=14):
    """{(cells, K): the traced rays of every pair, [n][6]}.  The host function is called once per pair (about
    0.6 ms each on the night scene), so the pairs are spread over worker processes, forked before the device is
    opened."""
    import multiprocessing as mp
    out = {}
    with mp.get_context("fork").Pool(workers) as pool:
        for cells, k in CONFIGS:
            info, _ = rt.light_grid_host(sc, cells)
            pairs = info.n[0] * info.n[1] * info.n[2] * info.n_lights
            step = max(1, (pairs + 8 * workers - 1) // (8 * workers))
            jobs = [(cells, k, seed, info.n_lights, lo, min(pairs, lo + step)) for lo in range(0, pairs, step)]
            out[(cells, k)] = np.concatenate(pool.map(_pair_chunk, jobs))
    return out


def cost(rt, torch, dev, stream, sc, seed, batches):
    from nee_measure import DEPTH, SPP, median_ms
    N = rt._native
    rows = []
    dev.upload(sc, "sah")
    cam = rt.default_camera(1200, "std3x2")
    buf = torch.zeros((cam.image_height, cam.image_width, 3), dtype=torch.float64, device="cuda")
    rs = rt.RenderSettings(samples=SPP, max_reflect=DEPTH, seed=seed)
    dev.light_sampling(N.RT_LIGHT_SAMPLE_SOLID_ANGLE)
    dev.light_pick(16)
    frame_ms, _ = median_ms(stream, lambda s: dev.render_nee_device(cam, rs, True, buf.data_ptr(), s))
    for cells, k in CONFIGS:
        info = dev.light_pick(cells)
        dev.light_visibility(k, seed)  # warm-up
        kernel, wall = [], []
        for _ in range(REPS):
            t = time.perf_counter()
            rep = dev.light_visibility(k, seed)
            wall.append((time.perf_counter() - t) * 1e3)
            kernel.append(rep.kernel_ms)
        masks = np.ascontiguousarray(dev.light_visibility_masks())
        cdf = np.zeros(masks.size)
        t = time.perf_counter()  # (the C call alone: the light list, the grid's shape, then the rows)
        code = N.rt_lib().rt_light_visibility_rows_host(sc.desc_ptr, cells, k, masks.ctypes.data, cdf.ctypes.data)
        rows_ms = (time.perf_counter() - t) * 1e3
        assert code == 0, code
        row = dict(cells=cells, rays=k, grid=list(info.n), lights=info.n_lights, pairs=int(rep.pairs),
                   traced=int(rep.traced), unoccluded=int(rep.unoccluded), dead_points=int(rep.dead_points),
                   kernel_ms=kernel, call_wall_ms=wall, rows_host_ms=rows_ms,
                   readback_upload_sync_ms=float(np.median(wall) - np.median(kernel) - rows_ms),
                   nee_frame_16spp_ms=frame_ms)
        batch = batches[(cells, k)]
        assert len(batch) == rep.traced
        d_rays = torch.from_numpy(batch).cuda()
        d_out = torch.zeros(len(batch), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        lib = N.rt_lib()

        def query(s):
            code = lib.rt_scene_occluded_device(dev.handle, d_rays.data_ptr(), len(batch), 0.001, 1.0 - 2.0 ** -20,
                                                None, d_out.data_ptr(), s)
            assert code == 0, code

        _, row["occluded_device_same_rays_ms"] = median_ms(stream, query, REPS)
        row["occluded_device_unoccluded"] = int((d_out == 0).sum().item())  # (== unoccluded minus the untraced bits)
        del d_rays, d_out
        log(row)
        rows.append(row)
    return rows


def payoff(rt, torch, dev, stream, sc, seed):
    from nee_measure import DEPTH, REF_BEGIN, REF_SPP, REF_STEP, SPP, SPPS, errors, median_ms
    N = rt._native
    dev.upload(sc, "sah")
    cam = rt.default_camera(1200, "std3x2")
    total = REF_BEGIN + REF_SPP
    dev.light_sampling(N.RT_LIGHT_SAMPLE_SOLID_ANGLE)

    def select(cells, k):
        dev.light_pick(cells)
        if k:
            dev.light_visibility(k, seed)

    rs = rt.RenderSettings(samples=SPP, max_reflect=DEPTH, seed=seed)
    buf = torch.zeros((cam.image_height, cam.image_width, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    row = dict(frame="random-night 1200x800", spp=SPP, max_depth=DEPTH, lights=len(dev.lights()[0]), ms={})
    row["render_ms"], _ = median_ms(stream, lambda s: dev.render_device(cam, rs, buf.data_ptr(), s))
    for key, cells, k in PASSES:
        select(cells, k)
        row["ms"][key], _ = median_ms(stream, lambda s: dev.render_nee_device(cam, rs, True, buf.data_ptr(), s))
    log(row)

    def ranged(begin, count):
        return rt.RenderSettings(samples=max(total, begin + count), max_reflect=DEPTH, seed=seed, sample_begin=begin,
                                 sample_count=count)

    ref = sum(dev.render(cam, ranged(b, REF_STEP)) for b in range(REF_BEGIN, total, REF_STEP)) / REF_SPP
    row["reference_spp"], row["reference_mean"], row["rows"] = REF_SPP, float(ref.mean()), []
    for S in SPPS:
        r = dict(spp=S, render=errors(dev.render(cam, ranged(0, S)) / S, ref))
        for key, cells, k in PASSES:
            select(cells, k)
            r[key] = errors(dev.render_nee(cam, ranged(0, S), mis=True) / S, ref)
            if k:
                eq = min(REF_BEGIN, max(1, int(round(S * row["ms"][key] / row["render_ms"]))))
                r["render_at_time_of_" + key] = dict(spp=eq, **errors(dev.render(cam, ranged(0, eq)) / eq, ref))
        log(r)
        row["rows"].append(r)
    return row


def lamps(rt, dev, seed):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import direct_ref as D
    import lightgrid_ref as G
    import test_gpu_light_visibility as T
    dev.upload(T.boxed_lamp_field().finalize(seed))
    dev.light_sampling(rt._native.RT_LIGHT_SAMPLE_AREA)
    cam = G.lamp_camera(32)
    out = {}
    for key, k in (("plain_grid", 0), ("visibility_8", 8)):
        dev.light_pick(4)
        if k:
            dev.light_visibility(k, seed)
        for mis in (False, True):
            frames = [dev.render_nee(cam, rt.RenderSettings(samples=256, max_reflect=4, seed=seed, sample_begin=16 * i,
                                                            sample_count=16), mis=mis) for i in range(16)]
            m, s = D.range_means(frames)
            out[key + ("_mis" if mis else "")] = dict(mean_per_sample=m / 16, standard_error_per_sample=s / 16)
    log(out)
    return out


def main():
    out = sys.argv[1]
    sys.path.insert(0, os.path.join(REPO, "shirley-raytracing-rs_amd"))
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import raytracer as rt
    import torch
    from nee_measure import SEED
    sc = rt.scenes.random_scene(SEED, night=True).finalize(SEED)
    batches = pair_rays(rt, sc, SEED)  # (before the device is opened: the workers are forked)
    dev = rt.Device(0)
    stream = torch.cuda.Stream()
    result = dict(cost=cost(rt, torch, dev, stream, sc, SEED, batches))
    del batches
    result["payoff"] = payoff(rt, torch, dev, stream, sc, SEED)
    result["lamps"] = lamps(rt, dev, SEED)
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
