#!/usr/bin/env python3
"""Measurements of the adaptive sampler for DESIGN.md §12 (needs an MI355X):

  overhead  rt_render_adaptive with threshold 0 (every tile in every step, so the step count is known)
            against rt_render with the same samples and sample_chunk, on the headline frame;
  payoff    for Cornell 600x600 and the headline frame: the threshold at which the adaptive frame's RMSE
            against a high-spp frame equals a uniform frame's at a fixed spp (bisection), with wall time and
            total samples of both.  RMSE is taken on the displayed value sqrt(clip(mean, 0, 1)) per channel.

usage: tools/adaptive_measure.py OUT.json [overhead] [payoff]
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "shirley-raytracing-rs_amd"))
import raytracer as rt  # noqa: E402

SEED = 0x5EED


def timed(fn, reps=3):
    out, ts = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def headline(dev):
    dev.upload(rt.scenes.random_scene(SEED).finalize(SEED), "sah")
    return rt.default_camera(1200, "std3x2")


def cornell(dev):
    dev.upload(rt.scenes.create_cornell_box().finalize(SEED), "sah")
    return rt.cornell_camera(600)


def overhead(dev):
    cam = headline(dev)
    res = []
    for samples, chunk, mn, step in ((512, 8, 64, 64), (512, 8, 256, 256), (512, 8, 32, 32)):
        s = rt.RenderSettings(samples=samples, seed=SEED, sample_chunk=chunk)
        dev.render(cam, s)  # warm-up
        _, t_uni = timed(lambda: dev.render(cam, s))
        uni_kernel = dev.counters().kernel_ms
        ad = rt.AdaptiveSettings(threshold=0.0, min_samples=mn, step=step)
        out, t_ad = timed(lambda: dev.render_adaptive(cam, s, ad))
        rep = out[4]
        res.append(dict(samples=samples, chunk=chunk, min_samples=mn, step=step, steps=rep.steps,
                        uniform_ms=t_uni, adaptive_ms=t_ad, uniform_kernel_ms=uni_kernel,
                        adaptive_kernel_ms=rep.kernel_ms, adaptive_fold_ms=rep.fold_ms,
                        ms_per_extra_step=(float(np.median(t_ad)) - float(np.median(t_uni))) / max(1, rep.steps - 1)))
        print(json.dumps(res[-1]), flush=True)
    return res


def shown(accum, counts):
    return np.sqrt(np.clip(accum / np.maximum(counts, 1)[..., None], 0.0, 1.0))


def payoff(dev):
    res = []
    for name, setup, gt_spp, uni_spp, chunk in (("cornell 600x600", cornell, 8192, 256, 16),
                                                 ("random 1200x800 (headline)", headline, 4096, 128, 8)):
        cam = setup(dev)
        h, w = cam.image_height, cam.image_width
        truth = shown(dev.render(cam, rt.RenderSettings(samples=gt_spp, seed=SEED + 1)), np.full((h, w), gt_spp))

        def rmse(img):
            return float(np.sqrt(np.mean((img - truth) ** 2)))

        s_uni = rt.RenderSettings(samples=uni_spp, seed=SEED, sample_chunk=chunk)
        uni, t_uni = timed(lambda: dev.render(cam, s_uni))
        target = rmse(shown(uni, np.full((h, w), uni_spp)))
        # two schedules: fine steps (2 batches first, then 4 at a time, up to 8x the uniform spp) and coarse
        # ones (half the uniform spp first and per step, up to 4x)
        for sched, mn, step, mx in (("fine", 2 * chunk, 4 * chunk, 8 * uni_spp),
                                    ("coarse", uni_spp // 2, uni_spp // 2, 4 * uni_spp)):
            s_ad = rt.RenderSettings(samples=mx, seed=SEED, sample_chunk=chunk)
            lo, hi, best = 0.0, 1.0, None
            trail = []
            for _ in range(10):  # bisection: the RMSE grows with the threshold
                thr = 0.5 * (lo + hi)
                ad = rt.AdaptiveSettings(threshold=thr, min_samples=mn, step=step, noise_floor=0.01)
                (accum, counts, _, _, rep), t_ad = timed(lambda: dev.render_adaptive(cam, s_ad, ad), reps=2)
                r = rmse(shown(accum, counts))
                trail.append(dict(threshold=thr, rmse=r, mean_spp=rep.samples / (w * h), samples=rep.samples,
                                  steps=rep.steps, ms=t_ad, kernel_ms=rep.kernel_ms, fold_ms=rep.fold_ms,
                                  spp_min=int(counts.min()), spp_max=int(counts.max())))
                if r <= target:
                    lo, best = thr, trail[-1]
                else:
                    hi = thr
            res.append(dict(frame=name, truth_spp=gt_spp, schedule=sched, min_samples=mn, step=step, max_spp=mx,
                            chunk=chunk, uniform=dict(spp=uni_spp, rmse=target, ms=t_uni, samples=w * h * uni_spp),
                            adaptive=best, trail=trail))
            print(json.dumps({k: v for k, v in res[-1].items() if k != "trail"}), flush=True)
    return res


def main():
    out = sys.argv[1]
    what = sys.argv[2:] or ["overhead", "payoff"]
    dev = rt.Device(0)
    result = {}
    if "overhead" in what:
        result["overhead"] = overhead(dev)
    if "payoff" in what:
        result["payoff"] = payoff(dev)
    dev.close()
    with open(out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
