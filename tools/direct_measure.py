#!/usr/bin/env python3
"""Measurements of the direct-lighting pass for DESIGN.md §15 (needs an MI355X; the product path only, no
oracle):

  timing   device time of rt_render_direct_device at 16 spp, chain 8 — HIP events on the call's stream, median
           of 5 after a warm-up call — on the 1200x800 headline frame (the day random scene: no listed light, so
           the pass is the walk to the vertex and the sky), the same frame of the night random scene (its
           FairyLight spheres listed) and the 600x600 Cornell box, next to rt_render_features_device and
           rt_render_ao_device (radius inf) on the same frames in the same process.
  payoff   on the Cornell box 600x600: the error of (a) emission + direct and (b) rt_render with max_depth = 2,
           each the mean over samples [0, S) for S in PAYOFF_SPP, against two REF_SPP-sample references of the
           direct-illumination frame, one per estimator, over samples [REF_BEGIN, REF_BEGIN + REF_SPP) (disjoint
           from every measured range): the RMSE over pixels and channels, the per-pixel error's median, 99th
           percentile and maximum, the share of pixels where (a) is closer than (b), and the pixels off by more
           than 1 (an area sample next to the lamp weighs 1 / distance^4: the estimator's outliers).  The two
           references are compared with each other.  Recorded, not asserted.

usage: tools/direct_measure.py OUT.json
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "shirley-raytracing-rs_amd"))
import raytracer as rt  # noqa: E402
import torch  # noqa: E402

SEED, SPP, CHAIN = 0x5EED, 16, 8
PAYOFF_SPP = (4, 16, 64)
REF_BEGIN, REF_SPP, REF_STEP = 1024, 16384, 2048


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


FRAMES = (
    ("random 1200x800 (headline)", lambda: rt.scenes.random_scene(SEED).finalize(SEED),
     lambda: rt.default_camera(1200, "std3x2")),
    ("random-night 1200x800", lambda: rt.scenes.random_scene(SEED, night=True).finalize(SEED),
     lambda: rt.default_camera(1200, "std3x2")),
    ("cornell 600x600", lambda: rt.scenes.create_cornell_box().finalize(SEED), lambda: rt.cornell_camera(600)),
)


def timing(dev, stream):
    res = []
    for name, make_scene, make_cam in FRAMES:
        dev.upload(make_scene(), "sah")
        cam = make_cam()
        h, w = cam.image_height, cam.image_width
        rs = rt.RenderSettings(samples=SPP, seed=SEED)
        vis = torch.zeros((h, w), dtype=torch.float64, device="cuda")
        alb = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
        nrm, dep, em, di = torch.zeros_like(alb), torch.zeros_like(vis), torch.zeros_like(alb), torch.zeros_like(alb)
        torch.cuda.synchronize()
        lights, unlisted = dev.lights()
        row = dict(frame=name, width=w, height=h, spp=SPP, chain=CHAIN, lights=len(lights), unlisted=unlisted,
                   wide_block=int(dev.stats().wide_block))
        row["features_ms"], row["features_ms_all"] = median_ms(stream, lambda s: dev.render_features_device(
            cam, rs, CHAIN, alb.data_ptr(), nrm.data_ptr(), dep.data_ptr(), s))
        row["ao_ms"], row["ao_ms_all"] = median_ms(stream, lambda s: dev.render_ao_device(
            cam, rs, CHAIN, float("inf"), vis.data_ptr(), s))
        row["direct_ms"], row["direct_ms_all"] = median_ms(stream, lambda s: dev.render_direct_device(
            cam, rs, CHAIN, em.data_ptr(), di.data_ptr(), s))
        row["mean_emission"] = float(em.mean().item()) / SPP
        row["mean_direct"] = float(di.mean().item()) / SPP
        print(json.dumps(row), file=sys.stderr, flush=True)
        res.append(row)
    return res


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def pixel_errors(a, ref):
    """Per-pixel error (RMS over the channels) -> its median, 99th percentile and maximum."""
    e = np.sqrt(np.mean((a - ref) ** 2, axis=2))
    q = np.percentile(e, [50, 99])
    return e, dict(median=float(q[0]), p99=float(q[1]), max=float(e.max()))


def payoff(dev):
    dev.upload(rt.scenes.create_cornell_box().finalize(SEED), "sah")
    cam = rt.cornell_camera(600)
    total = REF_BEGIN + REF_SPP

    def direct(begin, count):
        em, di = dev.render_direct(cam, rt.RenderSettings(samples=total, seed=SEED, sample_begin=begin,
                                                          sample_count=count), chain=CHAIN)
        return em + di

    def render2(begin, count):
        return dev.render(cam, rt.RenderSettings(samples=total, max_reflect=2, seed=SEED, sample_begin=begin,
                                                 sample_count=count))

    # two references over the same disjoint sample range, one per estimator
    ref_d = sum(direct(b, REF_STEP) for b in range(REF_BEGIN, total, REF_STEP)) / REF_SPP
    ref_r = sum(render2(b, REF_STEP) for b in range(REF_BEGIN, total, REF_STEP)) / REF_SPP
    _, between = pixel_errors(ref_d, ref_r)
    res = dict(frame="cornell 600x600", chain=CHAIN, reference_spp=REF_SPP, direct_reference_mean=float(ref_d.mean()),
               render2_reference_mean=float(ref_r.mean()), references_rmse=rmse(ref_d, ref_r),
               references_pixel_error=between, rows=[])
    for spp in PAYOFF_SPP:
        d, r = direct(0, spp) / spp, render2(0, spp) / spp
        row = dict(spp=spp)
        for name, ref in (("direct_reference", ref_d), ("render2_reference", ref_r)):
            ed, sd = pixel_errors(d, ref)
            er, sr = pixel_errors(r, ref)
            row[name] = dict(direct_rmse=rmse(d, ref), render2_rmse=rmse(r, ref), direct_pixel_error=sd,
                             render2_pixel_error=sr, pixels_where_direct_is_closer=float(np.mean(ed < er)),
                             direct_pixels_off_by_more_than_1=int(np.sum(ed > 1.0)),
                             render2_pixels_off_by_more_than_1=int(np.sum(er > 1.0)))
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["rows"].append(row)
    return res


def main():
    out = sys.argv[1]
    dev = rt.Device(0)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0  # (handle 0 would mean "the context's stream")
    result = dict(timing=timing(dev, stream), payoff=payoff(dev))
    dev.close()
    with open(out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
