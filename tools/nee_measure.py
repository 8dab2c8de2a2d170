#!/usr/bin/env python3
"""Measurements of the light-sampling path integrator for DESIGN.md §16 (needs an MI355X; the product path only,
no oracle):

  timing   device time of rt_render_device and of rt_render_nee_device with RT_NEE_MIS clear and set, at 16 spp
           and the scene's usual depth (50) — HIP events on the call's stream, median of 5 after a warm-up call,
           all passes in one process — on the Cornell box 600x600, the night random scene 1200x800 and box-light
           1200x800.
  error    per frame, against a REF_SPP-sample rt_render frame over samples [REF_BEGIN, REF_BEGIN + REF_SPP)
           (disjoint from every measured range): the error of the mean over samples [0, S) of rt_render and of
           rt_render_nee (both flag values) for S in SPPS (equal spp), and of rt_render at the sample count that
           fits rt_render_nee's time at S (equal time: S * nee_ms / render_ms, at least 1).  Per-pixel error = RMS
           over the channels; recorded: its median, 99th percentile and maximum, the frame RMSE and the count of
           pixels off by more than 1.  Recorded, not asserted.

usage: tools/nee_measure.py OUT.json
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "shirley-raytracing-rs_amd"))
import raytracer as rt  # noqa: E402
import torch  # noqa: E402

SEED, SPP, DEPTH = 0x5EED, 16, 50
SPPS = (4, 16, 64)
REF_BEGIN, REF_SPP, REF_STEP = 4096, 16384, 2048

FRAMES = (
    ("cornell 600x600", lambda: rt.scenes.create_cornell_box().finalize(SEED), lambda: rt.cornell_camera(600)),
    ("random-night 1200x800", lambda: rt.scenes.random_scene(SEED, night=True).finalize(SEED),
     lambda: rt.default_camera(1200, "std3x2")),
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


def errors(a, ref):
    e = np.sqrt(np.mean((a - ref) ** 2, axis=2))
    q = np.percentile(e, [50, 99])
    return dict(median=float(q[0]), p99=float(q[1]), max=float(e.max()), rmse=float(np.sqrt(np.mean((a - ref) ** 2))),
                pixels_off_by_more_than_1=int(np.sum(e > 1.0)), frame_mean=float(a.mean()))


def measure(dev, stream, name, make_scene, make_cam):
    dev.upload(make_scene(), "sah")
    cam = make_cam()
    h, w = cam.image_height, cam.image_width
    lights, unlisted = dev.lights()
    total = REF_BEGIN + REF_SPP
    rs = rt.RenderSettings(samples=SPP, max_reflect=DEPTH, seed=SEED)
    buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    row = dict(frame=name, width=w, height=h, spp=SPP, max_depth=DEPTH, lights=len(lights), unlisted=unlisted,
               wide_block=int(dev.stats().wide_block))
    row["render_ms"], row["render_ms_all"] = median_ms(stream, lambda s: dev.render_device(cam, rs, buf.data_ptr(), s))
    for mis in (False, True):
        key = "nee_mis_ms" if mis else "nee_ms"
        row[key], row[key + "_all"] = median_ms(stream, lambda s: dev.render_nee_device(cam, rs, mis, buf.data_ptr(), s))
    print(json.dumps(row), file=sys.stderr, flush=True)

    def ranged(begin, count):
        return rt.RenderSettings(samples=max(total, begin + count), max_reflect=DEPTH, seed=SEED, sample_begin=begin,
                                 sample_count=count)

    ref = sum(dev.render(cam, ranged(b, REF_STEP)) for b in range(REF_BEGIN, total, REF_STEP)) / REF_SPP
    row["reference_spp"], row["reference_mean"] = REF_SPP, float(ref.mean())
    row["rows"] = []
    for S in SPPS:
        r = dict(spp=S, render=errors(dev.render(cam, ranged(0, S)) / S, ref))
        for mis in (False, True):
            key = "nee_mis" if mis else "nee"
            r[key] = errors(dev.render_nee(cam, ranged(0, S), mis=mis) / S, ref)
            eq = min(REF_BEGIN, max(1, int(round(S * row[key + "_ms"] / row["render_ms"]))))
            r["render_equal_time_" + key] = dict(spp=eq, **errors(dev.render(cam, ranged(0, eq)) / eq, ref))
        print(json.dumps(r), file=sys.stderr, flush=True)
        row["rows"].append(r)
    return row


def main():
    out = sys.argv[1]
    dev = rt.Device(0)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0  # (handle 0 would mean "the context's stream")
    result = [measure(dev, stream, *f) for f in FRAMES]
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
