#!/usr/bin/env python3
"""Measurements of the spatially weighted light pick for DESIGN.md §18 (needs an MI355X; the product path only, no
oracle), by the protocol of tools/nee_measure.py:

  timing   device time of rt_render_device and of rt_render_nee_device (RT_NEE_MIS clear and set) with the
           uniform pick and with the light grid at CELLS cells, at 16 spp and depth 50 — HIP events on the call's
           stream, median of 5 after a warm-up call, all passes in one process, SAH tree — on the night random
           scene 1200x800 and on the Cornell box 600x600 (one light: the control, whose frames must not change and
           whose time shows the pick's pure overhead; cells = 1 against uniform there is the binary search's cost).
  error    per frame, against a REF_SPP-sample rt_render frame over samples [REF_BEGIN, REF_BEGIN + REF_SPP)
           (disjoint from every measured range): the error of the mean over samples [0, S) of rt_render and of
           every pass for S in SPPS, and of rt_render at the sample count that fits the pass's own time at S
           ("render = time": S * pass_ms / render_ms, at least 1).  Per-pixel error = RMS over the channels;
           recorded: its median, 99th percentile and maximum, the frame RMSE and the count of pixels off by more
           than 1.  Recorded, not asserted.

usage: tools/lightgrid_measure.py OUT.json
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "shirley-raytracing-rs_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import raytracer as rt  # noqa: E402
import torch  # noqa: E402
from nee_measure import DEPTH, REF_BEGIN, REF_SPP, REF_STEP, SEED, SPP, SPPS, errors, median_ms  # noqa: E402

CELLS = (0, 1, 4, 8, 16)  # 0: the uniform pick

FRAMES = (
    ("random-night 1200x800", lambda: rt.scenes.random_scene(SEED, night=True).finalize(SEED),
     lambda: rt.default_camera(1200, "std3x2")),
    ("cornell 600x600", lambda: rt.scenes.create_cornell_box().finalize(SEED), lambda: rt.cornell_camera(600)),
)


def pass_name(cells, mis):
    return ("uniform" if cells == 0 else f"cells{cells}") + ("_mis" if mis else "")


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
               wide_block=int(dev.stats().wide_block), grids={}, ms={}, ms_all={})
    row["render_ms"], row["render_ms_all"] = median_ms(stream, lambda s: dev.render_device(cam, rs, buf.data_ptr(), s))
    for cells in CELLS:
        info = dev.light_pick(cells)
        row["grids"][str(cells)] = dict(n=list(info.n), entries=info.n[0] * info.n[1] * info.n[2] * info.n_lights)
        for mis in (False, True):
            key = pass_name(cells, mis)
            row["ms"][key], row["ms_all"][key] = median_ms(
                stream, lambda s: dev.render_nee_device(cam, rs, mis, buf.data_ptr(), s))
    dev.light_pick(0)
    print(json.dumps({k: row[k] for k in ("frame", "render_ms", "ms", "grids")}), file=sys.stderr, flush=True)

    def ranged(begin, count):
        return rt.RenderSettings(samples=max(total, begin + count), max_reflect=DEPTH, seed=SEED, sample_begin=begin,
                                 sample_count=count)

    ref = sum(dev.render(cam, ranged(b, REF_STEP)) for b in range(REF_BEGIN, total, REF_STEP)) / REF_SPP
    row["reference_spp"], row["reference_mean"] = REF_SPP, float(ref.mean())
    row["rows"] = []
    frames = {}
    for S in SPPS:
        r = dict(spp=S, render=errors(dev.render(cam, ranged(0, S)) / S, ref))
        for cells in CELLS:
            dev.light_pick(cells)
            for mis in (False, True):
                key = pass_name(cells, mis)
                got = dev.render_nee(cam, ranged(0, S), mis=mis)
                frames[(S, cells, mis)] = got
                r[key] = errors(got / S, ref)
                eq = min(REF_BEGIN, max(1, int(round(S * row["ms"][key] / row["render_ms"]))))
                r["render_equal_time_" + key] = dict(spp=eq)
        dev.light_pick(0)
        for eq in sorted({v["spp"] for k, v in r.items() if k.startswith("render_equal_time_")}):
            e = errors(dev.render(cam, ranged(0, eq)) / eq, ref)
            for k, v in r.items():
                if k.startswith("render_equal_time_") and v["spp"] == eq:
                    v.update(e)
        print(json.dumps(r), file=sys.stderr, flush=True)
        row["rows"].append(r)
    # with one light every row of the grid is {1.0}: the frames are the uniform pick's, bit for bit
    row["grid_frames_equal_uniform"] = bool(all(
        np.array_equal(frames[(S, c, m)], frames[(S, 0, m)]) for S in SPPS for c in CELLS for m in (False, True)))
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
