#!/usr/bin/env python3
"""Measurements of the feature pass and the à-trous filter for DESIGN.md §13 (needs an MI355X):

  timing   for the headline frame (random_scene 1200x800) and Cornell 600x600 at 16 spp: the device time
           (HIP events on the call's stream, median of 5) of rt_render_features_device next to
           rt_render_device over the same sample range, and of rt_denoise_device with 1 .. 5 iterations.
           A call with k iterations runs dn_prepare, k dn_atrous launches (strides 1 .. 2^(k-1)) and
           dn_finish, so T(k) - T(k-1) is the dn_atrous launch at stride 2^(k-1) and T(1) holds prepare +
           the stride-1 launch + finish.
  quality  RMSE against a 4096-spp frame (seed + 1) on the per-channel means clipped to 1: the 16-spp frame,
           filtered without the colour term, and with it (the variance from rt_render_adaptive's moments at
           threshold 0, i.e. the uniform frame in batches of 4) at sigma_c 2 and 4; 3 iterations, the
           defaults otherwise.

usage: tools/denoise_measure.py OUT.json
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "shirley-raytracing-rs_amd"))
import raytracer as rt  # noqa: E402
import torch  # noqa: E402

SEED, SPP, TRUTH_SPP, BATCH, CHAIN = 0x5EED, 16, 4096, 4, 8


def headline(dev):
    dev.upload(rt.scenes.random_scene(SEED).finalize(SEED), "sah")
    return rt.default_camera(1200, "std3x2")


def cornell(dev):
    dev.upload(rt.scenes.create_cornell_box().finalize(SEED), "sah")
    return rt.cornell_camera(600)


STREAM = None  # a stream of torch's own: handle 0 (torch's default stream) would mean "the context's stream"


def device_ms(fn, reps=5):
    stream = STREAM
    fn(stream.cuda_stream)  # warm-up
    stream.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn(stream.cuda_stream)
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ts


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def measure(dev, name, setup):
    cam = setup(dev)
    h, w = cam.image_height, cam.image_width
    rs = rt.RenderSettings(samples=SPP, seed=SEED, sample_chunk=BATCH)
    acc = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    alb, nrm = torch.zeros_like(acc), torch.zeros_like(acc)
    dep = torch.zeros((h, w), dtype=torch.float64, device="cuda")
    out = torch.zeros_like(acc)
    torch.cuda.synchronize()
    render_ms, render_all = device_ms(lambda s: dev.render_device(cam, rs, acc.data_ptr(), s))
    feat_ms, feat_all = device_ms(lambda s: dev.render_features_device(cam, rs, CHAIN, alb.data_ptr(), nrm.data_ptr(),
                                                                       dep.data_ptr(), s))
    timing = dict(render_ms=render_ms, render_ms_all=render_all, render_kernel_ms=dev.counters().kernel_ms,
                  features_ms=feat_ms, features_ms_all=feat_all, denoise_ms={}, denoise_ms_all={})

    def filt(iterations, var=None, sigma_c=2.0, stream=0):
        dev.denoise_device(w, h, acc.data_ptr(), alb.data_ptr(), nrm.data_ptr(), dep.data_ptr(), out.data_ptr(),
                           samples=SPP, settings=rt.DenoiseSettings(iterations=iterations, sigma_c=sigma_c),
                           variance_ptr=0 if var is None else var.data_ptr(), stream=stream)

    for k in range(1, 6):
        timing["denoise_ms"][k], timing["denoise_ms_all"][k] = device_ms(lambda s: filt(k, stream=s))
    t = timing["denoise_ms"]
    timing["atrous_ms_by_stride"] = {1 << (k - 1): t[k] - t[k - 1] for k in range(2, 6)}

    # quality: the frame in batches of 4 with its moments (threshold 0: every tile takes every step)
    accum, counts, moments, _, _ = dev.render_adaptive(
        cam, rs, rt.AdaptiveSettings(threshold=0.0, min_samples=2 * BATCH, step=2 * BATCH))
    assert int(counts.min()) == int(counts.max()) == SPP
    truth = np.minimum(dev.render(cam, rt.RenderSettings(samples=TRUTH_SPP, seed=SEED + 1)) / TRUTH_SPP, 1.0)

    def rmse(sums):
        return float(np.sqrt(np.mean((np.minimum(sums / SPP, 1.0) - truth) ** 2)))

    acc.copy_(cuda(accum))
    var = cuda(rt.moments_variance(moments, counts, BATCH))
    torch.cuda.synchronize()
    quality = dict(noisy=rmse(accum))
    for label, v, sc in (("filtered_no_variance", None, 2.0), ("filtered_variance_sigma_c_2", var, 2.0),
                         ("filtered_variance_sigma_c_4", var, 4.0)):
        filt(3, v, sc, STREAM.cuda_stream)
        torch.cuda.synchronize()
        quality[label] = rmse(out.cpu().numpy())
    res = dict(frame=name, width=w, height=h, spp=SPP, truth_spp=TRUTH_SPP, chain=CHAIN, iterations=3,
               timing=timing, rmse=quality)
    print(json.dumps(res), flush=True)
    return res


def main():
    out = sys.argv[1]
    global STREAM
    dev = rt.Device(0)
    STREAM = torch.cuda.Stream()
    assert STREAM.cuda_stream != 0
    result = [measure(dev, "random 1200x800 (headline)", headline), measure(dev, "cornell 600x600", cornell)]
    dev.close()
    with open(out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
