#!/usr/bin/env python3
"""Measurements of the occlusion query and the ambient-occlusion pass for DESIGN.md §14 (needs an MI355X;
the product path only, no oracle):

  batches  ~10^6 bounce rays of the headline scene (the first hits of a 1200x800 frame's pixel-centre rays,
           t_max = inf) and ~10^6 Cornell bounce rays (1000x1000, t_max = 300): origin = the hit point,
           direction = the hit normal + a seeded random unit vector (numpy, from SEED).  Per node placement
           (auto, lds, global, half-lds) the device time of rt_scene_occluded_device — HIP events on the
           call's stream — for the any-hit instance and the traverse4 instance (SHIRLEY_OCCLUDED_CLOSEST=1),
           alternated call by call in one process: REPS timed calls each after a warm-up pair; median, minimum,
           maximum and quartiles.  The two instances' bytes are compared.
  variant  `--variant NAME=LIBDIR` repeats the batches in fresh child processes that load another build of the
           library (SHIRLEY_LIB_DIR; e.g. occluded4 compiled with -DRT_OCC_UNSORTED=0 by `tools/variant.sh sorted`),
           interleaved with child runs of the default build: default, variant, default, variant.
  ao       rt_render_ao_device at 16 spp, chain 8, on the headline frame (radius inf and 1) and on Cornell
           600x600 (radius inf and 300) next to rt_render_features_device on the same frames: median of 5.

usage: tools/occlusion_measure.py OUT.json [--variant NAME=LIBDIR]
       tools/occlusion_measure.py --batches   (a child run: prints one JSON line)
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "shirley-raytracing-rs_amd"))
import raytracer as rt  # noqa: E402
from raytracer import _native as N  # noqa: E402
import torch  # noqa: E402

SEED, REPS, SPP, CHAIN = 0x5EED, 20, 16, 8
PLACEMENTS = ("auto", "lds", "global", "half-lds")
HIT = np.dtype([("object", "<i4"), ("front_face", "<i4"), ("t", "<f8"), ("point", "<f8", 3), ("normal", "<f8", 3),
                ("u", "<f8"), ("v", "<f8")])
assert HIT.itemsize == C.sizeof(N.rt_hit)


def pixel_centre_rays(cam):
    """The pinhole rays through the pixel centres of `cam` (camera/mod.rs:97-131 without jitter and lens)."""
    o, u, v, w = (np.array(list(x)) for x in (cam.origin, cam.u, cam.v, cam.w))
    hor, ver = u * (cam.width * cam.focus_length), v * (cam.height * cam.focus_length)
    ll = o - hor * 0.5 - ver * 0.5 - w * (cam.focal_length * cam.focus_length)
    x, y = np.meshgrid((np.arange(cam.image_width) + 0.5) / cam.image_width,
                       (np.arange(cam.image_height) + 0.5) / cam.image_height)
    d = ll + x.reshape(-1, 1) * hor + y.reshape(-1, 1) * ver - o
    return np.hstack([np.broadcast_to(o, d.shape), d])


def bounce_rays(dev, cam, seed):
    rays = np.ascontiguousarray(pixel_centre_rays(cam))
    hits = np.zeros(len(rays), dtype=HIT)
    code = N.rt_lib().rt_scene_hit_ex(dev.handle, rays.ctypes.data, len(rays), 0.001, float("inf"),
                                      N.RT_TRAVERSAL_RENDER, C.cast(hits.ctypes.data, C.POINTER(N.rt_hit)))
    assert code == N.RT_OK
    hits = hits[hits["object"] >= 0]
    r = np.random.default_rng(seed).normal(size=(len(hits), 3))
    r /= np.linalg.norm(r, axis=1)[:, None]
    return np.ascontiguousarray(np.hstack([hits["point"], hits["normal"] + r]))


def stats(ts):
    q = np.percentile(ts, [25, 50, 75])
    return dict(median_ms=float(q[1]), min_ms=float(min(ts)), max_ms=float(max(ts)), q25_ms=float(q[0]),
                q75_ms=float(q[2]))


def time_call(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn(stream.cuda_stream)
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def set_instance(closest):
    if closest:
        os.environ["SHIRLEY_OCCLUDED_CLOSEST"] = "1"
    else:
        os.environ.pop("SHIRLEY_OCCLUDED_CLOSEST", None)


SCENES = {
    "headline": (lambda: rt.scenes.random_scene(SEED).finalize(SEED), lambda: rt.default_camera(1200, "std3x2"),
                 float("inf")),
    "cornell": (lambda: rt.scenes.create_cornell_box().finalize(SEED), lambda: rt.cornell_camera(1000), 300.0),
}


def batches(dev, stream):
    res = []
    for name, (make_scene, make_cam, t_max) in SCENES.items():
        scene = make_scene()
        dev.upload(scene, "sah")
        rays = bounce_rays(dev, make_cam(), SEED)
        r_dev = torch.from_numpy(rays).to("cuda")
        out = torch.zeros(len(rays), dtype=torch.uint8, device="cuda")
        for nodes in PLACEMENTS:
            dev.upload(scene, "sah", nodes)
            call = lambda s: dev.occluded_device(r_dev.data_ptr(), len(rays), out.data_ptr(), 0.001, t_max, 0, s)  # noqa: E731
            got = {}
            for closest in (False, True):  # warm-up pair, and the bytes
                set_instance(closest)
                time_call(stream, call)
                got[closest] = out.cpu().numpy().copy()
            ts = {False: [], True: []}
            for _ in range(REPS):
                for closest in (False, True):
                    set_instance(closest)
                    ts[closest].append(time_call(stream, call))
            set_instance(False)
            row = dict(batch=name, rays=len(rays), t_max=t_max, nodes=nodes, wide_block=int(dev.stats().wide_block),
                       occluded=int(got[False].sum()), same_bytes=bool(np.array_equal(got[False], got[True])),
                       any_hit=stats(ts[False]), closest_hit=stats(ts[True]))
            row["any_over_closest"] = row["any_hit"]["median_ms"] / row["closest_hit"]["median_ms"]
            print(json.dumps(row), file=sys.stderr, flush=True)
            res.append(row)
    return res


def median_ms(stream, fn, reps=5):
    time_call(stream, fn)
    ts = [time_call(stream, fn) for _ in range(reps)]
    return float(np.median(ts)), ts


def ao(dev, stream):
    res = []
    frames = (("random 1200x800 (headline)", SCENES["headline"][0], lambda: rt.default_camera(1200, "std3x2"),
               (float("inf"), 1.0)),
              ("cornell 600x600", SCENES["cornell"][0], lambda: rt.cornell_camera(600), (float("inf"), 300.0)))
    for name, make_scene, make_cam, radii in frames:
        dev.upload(make_scene(), "sah")
        cam = make_cam()
        h, w = cam.image_height, cam.image_width
        rs = rt.RenderSettings(samples=SPP, seed=SEED)
        vis = torch.zeros((h, w), dtype=torch.float64, device="cuda")
        alb = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
        nrm, dep = torch.zeros_like(alb), torch.zeros_like(vis)
        torch.cuda.synchronize()
        row = dict(frame=name, width=w, height=h, spp=SPP, chain=CHAIN, ao_ms={}, ao_ms_all={}, mean_visibility={})
        row["features_ms"], row["features_ms_all"] = median_ms(stream, lambda s: dev.render_features_device(
            cam, rs, CHAIN, alb.data_ptr(), nrm.data_ptr(), dep.data_ptr(), s))
        for radius in radii:
            key = str(radius)
            row["ao_ms"][key], row["ao_ms_all"][key] = median_ms(
                stream, lambda s: dev.render_ao_device(cam, rs, CHAIN, radius, vis.data_ptr(), s))
            row["mean_visibility"][key] = float(vis.mean().item()) / SPP
        print(json.dumps(row), file=sys.stderr, flush=True)
        res.append(row)
    return res


def child_batches(lib_dir):
    env = dict(os.environ)
    env.pop("SHIRLEY_OCCLUDED_CLOSEST", None)
    if lib_dir:
        env["SHIRLEY_LIB_DIR"] = os.path.abspath(lib_dir)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--batches"], env=env, capture_output=True, text=True,
                       timeout=900)
    if r.returncode:
        sys.stderr.write(r.stderr)
        raise SystemExit(f"child run ({lib_dir or 'default'}) failed with status {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    args = sys.argv[1:]
    if args == ["--batches"]:
        dev = rt.Device(0)
        stream = torch.cuda.Stream()
        print(json.dumps(batches(dev, stream)), flush=True)
        dev.close()
        return
    out, variant = args[0], None
    if len(args) == 3 and args[1] == "--variant":
        variant = args[2].split("=", 1)
    result = {}
    if variant:  # the children first, one GPU process at a time
        result["child_runs"] = []
        for label, lib_dir in (("default", None), (variant[0], variant[1])) * 2:
            result["child_runs"].append(dict(build=label, batches=child_batches(lib_dir)))
    dev = rt.Device(0)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0  # (handle 0 would mean "the context's stream")
    result["batches"] = batches(dev, stream)
    result["ao"] = ao(dev, stream)
    dev.close()
    with open(out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
