#!/usr/bin/env python3
"""Measurements of the adaptive light-sampling render for DESIGN.md §22 (needs an MI355X):

  overhead  rt_render_nee_adaptive_device with threshold 0 (every tile renders every sample) against
            rt_render_nee_device at the same spp: Cornell 600x600 and box-light 1200x800, 64 spp, RT_NEE_MIS set,
            medians of five event-timed calls after a warm-up.  The difference is the cost of the counter, the
            per-batch stores and the checks;
  fetch     those frames and a mixed-threshold frame with the default grid (the device's fill), then with
            SHIRLEY_NEE_BLOCKS set to one block per block's worth of tiles — the uniform kernel's grid, above the
            fill on these frames — so that there are as many waves as tiles;
  payoff    DESIGN.md §12's method on Cornell 600x600: the threshold at which the adaptive frame's RMSE against a
            16384-spp rt_render frame over a disjoint sample range equals a uniform rt_render_nee frame's at a
            fixed spp (bisection), with the samples and the device time of both, for a few schedules.  RMSE is
            taken on the displayed value sqrt(clip(mean, 0, 1)) per channel.

usage: tools/nee_adaptive_measure.py OUT.json [overhead] [fetch] [payoff]
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "shirley-raytracing-rs_amd"))
import raytracer as rt  # noqa: E402
import torch  # noqa: E402

SEED, DEPTH, SPP, B = 0x5EED, 50, 64, 4
REF_BEGIN, REF_SPP, REF_STEP = 4096, 16384, 2048

FRAMES = (
    ("cornell 600x600", lambda: rt.scenes.create_cornell_box().finalize(SEED), lambda: rt.cornell_camera(600)),
    ("box-light 1200x800", lambda: rt.scenes.create_box_light().finalize(SEED),
     lambda: rt.scene_camera("box-light", 1200, "std3x2")),
)


def time_call(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn(stream.cuda_stream)
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(stream, fn, reps=5):
    time_call(stream, fn)
    ts = [time_call(stream, fn) for _ in range(reps)]
    return float(np.median(ts)), ts


class Buffers:
    def __init__(self, cam):
        h, w = cam.image_height, cam.image_width
        self.h, self.w = h, w
        self.accum = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
        self.moments = torch.zeros((h, w, 2), dtype=torch.float64, device="cuda")
        self.counts = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        self.err = torch.zeros(((h + 7) // 8, (w + 7) // 8), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

    def adaptive(self, dev, cam, rs, ad, s):
        dev.render_nee_adaptive_device(cam, rs, ad, True, self.accum.data_ptr(), self.counts.data_ptr(),
                                       self.moments.data_ptr(), self.err.data_ptr(), s)


def settings(spp):
    return rt.RenderSettings(samples=spp, max_reflect=DEPTH, seed=SEED, sample_chunk=B)


def with_blocks(n, fn):
    old = os.environ.pop("SHIRLEY_NEE_BLOCKS", None)
    if n:
        os.environ["SHIRLEY_NEE_BLOCKS"] = str(n)
    try:
        return fn()
    finally:
        os.environ.pop("SHIRLEY_NEE_BLOCKS", None)
        if old is not None:
            os.environ["SHIRLEY_NEE_BLOCKS"] = old


def overhead_and_fetch(dev, stream, what):
    res = []
    for name, make_scene, make_cam in FRAMES:
        dev.upload(make_scene(), "sah")
        cam = make_cam()
        buf = Buffers(cam)
        rs = settings(SPP)
        tiles = buf.err.numel()
        per_block = 16 if dev.stats().wide_block else 4
        one_tile_per_wave = (tiles + per_block - 1) // per_block
        row = dict(frame=name, spp=SPP, max_depth=DEPTH, batch=B, tiles=tiles, wide_block=int(dev.stats().wide_block),
                   blocks_one_tile_per_wave=one_tile_per_wave)
        row["nee_ms"], row["nee_ms_all"] = median_ms(
            stream, lambda s: dev.render_nee_device(cam, rs, True, buf.accum.data_ptr(), s))
        for label, thr, mn, step in (("threshold_0", 0.0, 16, 16), ("threshold_0_fine", 0.0, 8, 4),
                                     ("mixed", 0.05, 16, 8)):
            ad = rt.AdaptiveSettings(threshold=thr, min_samples=mn, step=step, noise_floor=0.01)
            r = dict(threshold=thr, min_samples=mn, step=step)
            r["ms"], r["ms_all"] = median_ms(stream, lambda s: buf.adaptive(dev, cam, rs, ad, s))
            r["mean_spp"] = float(buf.counts.double().mean().item())
            if "fetch" in what:
                r["ms_one_tile_per_wave"], r["ms_one_tile_per_wave_all"] = with_blocks(
                    one_tile_per_wave, lambda: median_ms(stream, lambda s: buf.adaptive(dev, cam, rs, ad, s)))
            row[label] = r
        row["overhead_ms"] = row["threshold_0"]["ms"] - row["nee_ms"]
        print(json.dumps(row), file=sys.stderr, flush=True)
        res.append(row)
    return res


def shown(accum, counts):
    return np.sqrt(np.clip(accum / np.maximum(counts, 1)[..., None], 0.0, 1.0))


def payoff(dev, stream):
    name, make_scene, make_cam = FRAMES[0]
    dev.upload(make_scene(), "sah")
    cam = make_cam()
    buf = Buffers(cam)
    h, w = buf.h, buf.w
    total = REF_BEGIN + REF_SPP

    def ranged(begin, count):
        return rt.RenderSettings(samples=total, max_reflect=DEPTH, seed=SEED, sample_begin=begin, sample_count=count)

    ref = sum(dev.render(cam, ranged(b, REF_STEP)) for b in range(REF_BEGIN, total, REF_STEP))
    truth = shown(ref, np.full((h, w), REF_SPP))

    def rmse(img):
        return float(np.sqrt(np.mean((img - truth) ** 2)))

    res = []
    for uni_spp in (64, 256):
        rs_uni = settings(uni_spp)
        t_uni, t_uni_all = median_ms(stream, lambda s: dev.render_nee_device(cam, rs_uni, True, buf.accum.data_ptr(), s))
        target = rmse(shown(buf.accum.cpu().numpy(), np.full((h, w), uni_spp)))
        for sched, mn, step, mx in (("fine", 2 * B, 2 * B, 4 * uni_spp), ("quarter", uni_spp // 4, uni_spp // 4, 4 * uni_spp),
                                    ("half", uni_spp // 2, uni_spp // 2, 4 * uni_spp)):
            rs_ad = settings(mx)
            lo, hi, best, trail = 0.0, 1.0, None, []
            for _ in range(9):  # bisection: the RMSE grows with the threshold
                thr = 0.5 * (lo + hi)
                ad = rt.AdaptiveSettings(threshold=thr, min_samples=mn, step=step, noise_floor=0.01)
                ms, ms_all = median_ms(stream, lambda s: buf.adaptive(dev, cam, rs_ad, ad, s), reps=3)
                counts = buf.counts.cpu().numpy()
                r = rmse(shown(buf.accum.cpu().numpy(), counts))
                trail.append(dict(threshold=thr, rmse=r, mean_spp=float(counts.mean()), samples=int(counts.sum()), ms=ms,
                                  ms_all=ms_all, spp_min=int(counts.min()), spp_max=int(counts.max())))
                if r <= target:
                    lo, best = thr, trail[-1]
                else:
                    hi = thr
            res.append(dict(frame=name, truth_spp=REF_SPP, schedule=sched, min_samples=mn, step=step, max_spp=mx, batch=B,
                            uniform=dict(spp=uni_spp, rmse=target, ms=t_uni, ms_all=t_uni_all, samples=w * h * uni_spp),
                            adaptive=best, trail=trail))
            print(json.dumps({k: v for k, v in res[-1].items() if k != "trail"}), file=sys.stderr, flush=True)
    return res


def main():
    out = sys.argv[1]
    what = sys.argv[2:] or ["overhead", "fetch", "payoff"]
    dev = rt.Device(0)
    stream = torch.cuda.Stream()
    result = {}
    with torch.cuda.stream(stream):
        if "overhead" in what or "fetch" in what:
            result["overhead_and_fetch"] = overhead_and_fetch(dev, stream, what)
        if "payoff" in what:
            result["payoff"] = payoff(dev, stream)
    dev.close()
    with open(out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
