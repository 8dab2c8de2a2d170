#!/usr/bin/env python3
"""Measurements of solid-angle sampling of sphere lights for DESIGN.md §19 (needs an MI355X; the product path
only, no oracle), by the protocol of tools/lightgrid_measure.py:

  cost     device time of rt_render_nee_device (RT_NEE_MIS clear and set) in mode AREA and in mode SOLID_ANGLE at
           16 spp and depth 50 — HIP events on the call's stream, sets of 5 after a warm-up call, SAH tree, uniform
           pick — on the night random scene 1200x800, the Cornell box 600x600 (no sphere light: the control) and
           the tests' lamp field at 600x600.  Every set runs in a fresh child process; with PARENT_TREE (a checkout
           of the parent commit with its libraries built) its AREA sets alternate with this tree's, ROUNDS times.
  payoff   night random 1200x800, against a REF_SPP-sample rt_render frame over samples
           [REF_BEGIN, REF_BEGIN + REF_SPP) (disjoint from every measured range): the error of the mean over
           samples [0, S), S in SPPS, of rt_render, of rt_render_nee with area + uniform pick, cone + uniform pick
           and cone + 16 cells (both RT_NEE_MIS values), and of rt_render at the sample count that fits the time
           of cone + 16 cells.  Per-pixel error = RMS over the channels; recorded: its median, 99th percentile and
           maximum, the frame RMSE and the count of pixels off by more than 1.  Recorded, not asserted.

usage: tools/cone_measure.py OUT.json [PARENT_TREE]
       tools/cone_measure.py --cost-set TREE        (a child: one set per frame and pass, JSON on stdout)
"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 5
GRID = 16


def frames(rt, seed):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import lightgrid_ref as G
    return (
        ("random-night 1200x800", lambda: rt.scenes.random_scene(seed, night=True).finalize(seed),
         lambda: rt.default_camera(1200, "std3x2")),
        ("cornell 600x600", lambda: rt.scenes.create_cornell_box().finalize(seed), lambda: rt.cornell_camera(600)),
        ("lamp-field 600x600", lambda: G.lamp_field().finalize(seed), lambda: G.lamp_camera(600)),
    )


def cost_set(tree):
    """One set of 5 per frame, mode and flag value, with the libraries and the Python package of `tree`."""
    sys.path.insert(0, os.path.join(tree, "shirley-raytracing-rs_amd"))
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import raytracer as rt
    import torch
    from nee_measure import DEPTH, SEED, SPP, median_ms
    dev = rt.Device(0)
    stream = torch.cuda.Stream()
    modes = ("area", "cone") if hasattr(dev, "light_sampling") else ("area",)
    out = {}
    for name, make_scene, make_cam in frames(rt, SEED):
        dev.upload(make_scene(), "sah")
        cam = make_cam()
        rs = rt.RenderSettings(samples=SPP, max_reflect=DEPTH, seed=SEED)
        buf = torch.zeros((cam.image_height, cam.image_width, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        row = out[name] = {}
        for mode in modes:
            if len(modes) > 1:
                dev.light_sampling(modes.index(mode))
            for mis in (False, True):
                med, ts = median_ms(stream, lambda s: dev.render_nee_device(cam, rs, mis, buf.data_ptr(), s))
                row[mode + ("_mis" if mis else "")] = ts
            if mode == "area":
                row["checksum_area_mis"] = float(buf.sum().item())
    dev.close()
    print(json.dumps(out))


def child(tree):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cost-set", tree], capture_output=True, text=True,
                       timeout=300)
    if r.returncode:
        raise SystemExit(f"cost set of {tree} failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def payoff():
    sys.path.insert(0, os.path.join(REPO, "shirley-raytracing-rs_amd"))
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import raytracer as rt
    import torch
    from nee_measure import DEPTH, REF_BEGIN, REF_SPP, REF_STEP, SEED, SPP, SPPS, errors, median_ms
    N = rt._native
    dev = rt.Device(0)
    stream = torch.cuda.Stream()
    name, make_scene, make_cam = frames(rt, SEED)[0]
    dev.upload(make_scene(), "sah")
    cam = make_cam()
    total = REF_BEGIN + REF_SPP
    passes = (("area_uniform", N.RT_LIGHT_SAMPLE_AREA, 0), ("cone_uniform", N.RT_LIGHT_SAMPLE_SOLID_ANGLE, 0),
              (f"cone_cells{GRID}", N.RT_LIGHT_SAMPLE_SOLID_ANGLE, GRID))

    def select(mode, cells):
        dev.light_pick(cells)
        dev.light_sampling(mode)

    rs = rt.RenderSettings(samples=SPP, max_reflect=DEPTH, seed=SEED)
    buf = torch.zeros((cam.image_height, cam.image_width, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    row = dict(frame=name, spp=SPP, max_depth=DEPTH, lights=len(dev.lights()[0]), ms={})
    row["render_ms"], _ = median_ms(stream, lambda s: dev.render_device(cam, rs, buf.data_ptr(), s))
    for key, mode, cells in passes:
        select(mode, cells)
        for mis in (False, True):
            row["ms"][key + ("_mis" if mis else "")], _ = median_ms(
                stream, lambda s: dev.render_nee_device(cam, rs, mis, buf.data_ptr(), s))
    print(json.dumps(row), file=sys.stderr, flush=True)

    def ranged(begin, count):
        return rt.RenderSettings(samples=max(total, begin + count), max_reflect=DEPTH, seed=SEED, sample_begin=begin,
                                 sample_count=count)

    ref = sum(dev.render(cam, ranged(b, REF_STEP)) for b in range(REF_BEGIN, total, REF_STEP)) / REF_SPP
    row["reference_spp"], row["reference_mean"], row["rows"] = REF_SPP, float(ref.mean()), []
    for S in SPPS:
        r = dict(spp=S, render=errors(dev.render(cam, ranged(0, S)) / S, ref))
        for key, mode, cells in passes:
            select(mode, cells)
            for mis in (False, True):
                r[key + ("_mis" if mis else "")] = errors(dev.render_nee(cam, ranged(0, S), mis=mis) / S, ref)
        eq = min(REF_BEGIN, max(1, int(round(S * row["ms"][f"cone_cells{GRID}_mis"] / row["render_ms"]))))
        r["render_equal_time"] = dict(spp=eq, **errors(dev.render(cam, ranged(0, eq)) / eq, ref))
        print(json.dumps(r), file=sys.stderr, flush=True)
        row["rows"].append(r)
    dev.close()
    return row


def main():
    if sys.argv[1] == "--cost-set":
        return cost_set(sys.argv[2])
    out = sys.argv[1]
    parent = sys.argv[2] if len(sys.argv) > 2 else None
    result = dict(cost=dict(rounds=ROUNDS, new=[], parent=[]))
    for _ in range(ROUNDS):  # the two trees alternate, each set in a fresh process
        if parent:
            result["cost"]["parent"].append(child(parent))
        result["cost"]["new"].append(child(REPO))
        print(json.dumps(result["cost"]["new"][-1]), file=sys.stderr, flush=True)
    result["payoff"] = payoff()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
