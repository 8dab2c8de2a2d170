#!/usr/bin/env python3
"""Measurements of solid-angle sampling of rect lights for DESIGN.md §20 (needs an MI355X; the product path only, no
oracle), by the protocol of tools/nee_measure.py and tools/cone_measure.py, all in one process on the Cornell box
600x600 (one rect light), SAH tree, uniform pick:

  cost     device time of rt_render_device, of rt_render_nee_device (RT_NEE_MIS clear and set) and of
           rt_render_direct_device in mode AREA and in mode SOLID_ANGLE_ALL at 16 spp (depth 50; direct: chain 8) —
           HIP events on the call's stream, sets of 5 after a warm-up call, the two modes alternated ROUNDS times.
  payoff   against a REF_SPP-sample rt_render frame over samples [REF_BEGIN, REF_BEGIN + REF_SPP) (disjoint from
           every measured range): the error of the mean over samples [0, S), S in SPPS, of rt_render, of
           rt_render_nee in both modes (both RT_NEE_MIS values), and of rt_render at the sample count that fits the
           time of mode 3 with RT_NEE_MIS.  Per-pixel error = RMS over the channels; recorded: its median, 99th
           percentile and maximum, the frame RMSE and the count of pixels off by more than 1.  Recorded, not asserted.

usage: tools/rect_measure.py OUT.json
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
ROUNDS = 3


def main():
    from nee_measure import DEPTH, REF_BEGIN, REF_SPP, REF_STEP, SEED, SPP, SPPS, errors, median_ms, rt, torch
    N = rt._native
    modes = (("area", N.RT_LIGHT_SAMPLE_AREA), ("solid_angle_all", N.RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL))
    out = sys.argv[1]
    dev = rt.Device(0)
    stream = torch.cuda.Stream()
    dev.upload(rt.scenes.create_cornell_box().finalize(SEED), "sah")
    cam = rt.cornell_camera(600)
    rs = rt.RenderSettings(samples=SPP, max_reflect=DEPTH, seed=SEED)
    buf = torch.zeros((cam.image_height, cam.image_width, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    row = dict(frame="cornell 600x600", spp=SPP, max_depth=DEPTH, lights=len(dev.lights()[0]),
               wide_block=int(dev.stats().wide_block), rounds=ROUNDS, ms={})
    row["render_ms"], row["render_ms_all"] = median_ms(stream, lambda s: dev.render_device(cam, rs, buf.data_ptr(), s))
    for _ in range(ROUNDS):
        for key, mode in modes:
            dev.light_sampling(mode)
            for mis in (False, True):
                _, ts = median_ms(stream, lambda s: dev.render_nee_device(cam, rs, mis, buf.data_ptr(), s))
                row["ms"].setdefault(f"nee_{key}" + ("_mis" if mis else ""), []).append(ts)
            _, ts = median_ms(stream, lambda s: dev.render_direct_device(cam, rs, 8, 0, buf.data_ptr(), s))
            row["ms"].setdefault(f"direct_{key}", []).append(ts)
    print(json.dumps(row), file=sys.stderr, flush=True)

    def median(key):
        import numpy as np
        return float(np.median([np.median(ts) for ts in row["ms"][key]]))

    total = REF_BEGIN + REF_SPP

    def ranged(begin, count):
        return rt.RenderSettings(samples=max(total, begin + count), max_reflect=DEPTH, seed=SEED, sample_begin=begin,
                                 sample_count=count)

    ref = 0.0
    for b in range(REF_BEGIN, total, REF_STEP):
        ref = ref + dev.render(cam, ranged(b, REF_STEP))
        print(f"reference: {b + REF_STEP - REF_BEGIN} of {REF_SPP} spp", file=sys.stderr, flush=True)
    ref = ref / REF_SPP
    row["reference_spp"], row["reference_mean"], row["rows"] = REF_SPP, float(ref.mean()), []
    for S in SPPS:
        r = dict(spp=S, render=errors(dev.render(cam, ranged(0, S)) / S, ref))
        for key, mode in modes:
            dev.light_sampling(mode)
            for mis in (False, True):
                r[f"nee_{key}" + ("_mis" if mis else "")] = errors(dev.render_nee(cam, ranged(0, S), mis=mis) / S, ref)
        eq = min(REF_BEGIN, max(1, int(round(S * median("nee_solid_angle_all_mis") / row["render_ms"]))))
        r["render_equal_time"] = dict(spp=eq, **errors(dev.render(cam, ranged(0, eq)) / eq, ref))
        print(json.dumps(r), file=sys.stderr, flush=True)
        row["rows"].append(r)
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
