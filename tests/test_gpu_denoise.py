"""rt_denoise_device (denoise.hip) against rt_denoise (the host function: the same denoise.h arithmetic): bit
for bit on the synthetic frames of tests/test_denoise.py and on a real GPU frame with GPU features; the
moments-to-variance helper on the device; and ray-cli --denoise against the Python pipeline built from the
same calls."""
import os
import subprocess

import numpy as np
import pytest
import torch

import denoise_ref as R
import raytracer as rt
from raytracer import _native as N

pytestmark = pytest.mark.gpu
SEED = 0x5EED


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def denoise_on_device(gpu, accum, albedo, normal, depth, settings, samples=0, feature_samples=0, counts=None,
                      variance=None):
    h, w, _ = accum.shape
    t = [dev(np.asarray(x, dtype=np.float64)) for x in (accum, albedo, normal, depth)]
    cn = None if counts is None else dev(np.asarray(counts, dtype=np.int32))
    va = None if variance is None else dev(np.asarray(variance, dtype=np.float64))
    out = torch.full((h, w, 3), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.denoise_device(w, h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), out.data_ptr(),
                       samples=samples, feature_samples=feature_samples, settings=settings,
                       counts_ptr=0 if cn is None else cn.data_ptr(), variance_ptr=0 if va is None else va.data_ptr(),
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def frames():
    return {(w, h): R.synthetic(w, h) for w, h in R.SIZES}


@pytest.mark.parametrize("iterations", R.ITERATIONS)
@pytest.mark.parametrize("size", R.SIZES)
def test_device_filter_equals_the_host_filter_bit_for_bit(gpu, frames, size, iterations):
    f = frames[size]
    S = rt.DenoiseSettings(iterations=iterations)
    for use_counts in (False, True):
        for use_variance in (False, True):
            accum, kw = R.case_arrays(f, use_counts, use_variance)
            host = rt.denoise(accum, f["albedo"], f["normal"], f["depth"], settings=S, **kw)
            got = denoise_on_device(gpu, accum, f["albedo"], f["normal"], f["depth"], S, **kw)
            assert R.same_bits(got, host), (size, iterations, use_counts, use_variance)


def test_device_filter_copies_non_finite_and_count_zero_pixels_like_the_host(gpu, frames):
    f = frames[(37, 21)]
    accum, kw = R.case_arrays(f, True, True)
    accum = accum.copy()
    accum[3, 5, 2] = np.nan
    accum[10, 30, 0] = np.inf
    S = rt.DenoiseSettings(iterations=3)
    host = rt.denoise(accum, f["albedo"], f["normal"], f["depth"], settings=S, **kw)
    got = denoise_on_device(gpu, accum, f["albedo"], f["normal"], f["depth"], S, **kw)
    ok = np.isfinite(host)
    assert np.array_equal(ok, np.isfinite(got)) and R.same_bits(got[ok], host[ok])
    assert np.array_equal(np.isnan(got), np.isnan(host))
    j, i = np.argwhere(f["counts"] == 0)[0]
    assert np.all(got[j, i] == 0.0)


def test_device_argument_rules(gpu, frames):
    f = frames[(8, 8)]
    accum, kw = R.case_arrays(f, False, False)
    for bad in (dict(iterations=9), dict(iterations=-1), dict(sigma_z=0.0), dict(sigma_a=-1.0), dict(sigma_c=0.0),
                dict(albedo_floor=0.0), dict(normal_power_log2=17)):
        with pytest.raises(rt.RtError) as e:
            denoise_on_device(gpu, accum, f["albedo"], f["normal"], f["depth"], rt.DenoiseSettings(**bad), **kw)
        assert e.value.code == N.RT_E_INVALID
    with pytest.raises(rt.RtError):
        denoise_on_device(gpu, accum, f["albedo"], f["normal"], f["depth"], rt.DenoiseSettings(), samples=0,
                          feature_samples=4)


def test_real_frame_with_gpu_features(gpu):
    scene = rt.scenes.random_scene(SEED).finalize(SEED)
    cam = rt.CameraBuilder(width=44, aspect_ratio=(44, 28), vfov=20.0, focal_length=1.0, aperture=0.001).build(
        rt.CameraPosition((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), focus_length=10.0))
    gpu.upload(scene)
    rs = rt.RenderSettings(samples=8, seed=SEED, sample_chunk=8)
    accum = gpu.render(cam, rs)
    albedo, normal, depth = gpu.render_features(cam, rs, chain=8)
    for S in (rt.DenoiseSettings(), rt.DenoiseSettings(iterations=5, sigma_z=0.1)):
        host = rt.denoise(accum, albedo, normal, depth, samples=8, settings=S)
        got = denoise_on_device(gpu, accum, albedo, normal, depth, S, samples=8)
        assert np.all(np.isfinite(host)) and R.same_bits(got, host)
        assert not np.array_equal(host, accum)


def test_moments_variance_device_equals_host(gpu):
    rng = np.random.default_rng(4)
    h, w, b = 13, 21, 4
    counts = (rng.integers(0, 7, size=(h, w)) * b).astype(np.int32)   # 0 and 1 batch included: NaN
    y = rng.uniform(0.0, 12.0, size=(h, w, 6))
    k = np.arange(6)[None, None, :] < (counts // b)[..., None]
    moments = np.stack([(y * k).sum(-1), (y * y * k).sum(-1)], axis=-1)
    host = rt.moments_variance(moments, counts, b)
    dm, dc = dev(moments), dev(counts)
    out = torch.zeros((h, w), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.moments_variance_device(dm.data_ptr(), dc.data_ptr(), b, w, h, out.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(host)) and np.array_equal(np.isnan(host), counts < 2 * b)
    ok = ~np.isnan(host)
    assert R.same_bits(got[ok], host[ok])


# ---- ray-cli ----------------------------------------------------------------------------------------
def run_cli(*args):
    r = subprocess.run([os.path.join(N.BIN_DIR, "ray-cli"), "render", *args], capture_output=True, text=True)
    return r


def test_cli_denoise_equals_the_python_pipeline(gpu, tmp_path):
    from PIL import Image
    out = str(tmp_path / "cornell.png")
    r = run_cli("cornell", "-w", "48", "-s", "16", "--seed", hex(SEED), "--denoise", "3", "-o", out)
    assert r.returncode == 0, r.stderr
    cam = rt.scene_camera("cornell", 48, "square")
    gpu.upload(rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED))
    rs = rt.RenderSettings(samples=16, seed=SEED)
    accum = gpu.render(cam, rs)
    albedo, normal, depth = gpu.render_features(cam, rs, chain=8)
    filtered = rt.denoise(accum, albedo, normal, depth, samples=16, settings=rt.DenoiseSettings(iterations=3))
    assert np.array_equal(np.asarray(Image.open(out)), rt.to_image(filtered, 16))
    assert not np.array_equal(rt.to_image(filtered, 16), rt.to_image(accum, 16))
    # `--denoise` alone means 3 iterations; the next option is not taken for its count
    out2 = str(tmp_path / "cornell_default.png")
    r = run_cli("cornell", "-w", "48", "-s", "16", "--seed", hex(SEED), "-o", out2, "--denoise")
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(out2)), np.asarray(Image.open(out)))


def test_cli_adaptive_denoise_with_variance_equals_the_python_pipeline(gpu, tmp_path):
    from PIL import Image
    out = str(tmp_path / "adaptive.png")
    b, mn, step, mx, thr, floor = 4, 8, 8, 32, 0.2, 0.01
    r = run_cli("random", "-w", "96", "-s", str(mx), "--seed", hex(SEED), "--camera-aspect-ratio", "std16x9",
                "--sample-chunk", str(b), "--adaptive", str(thr), "--min-samples", str(mn), "--adaptive-step",
                str(step), "--noise-floor", str(floor), "--denoise", "3", "--denoise-variance", "-o", out)
    assert r.returncode == 0, r.stderr
    cam = rt.scene_camera("random", 96, "std16x9")
    gpu.upload(rt.scenes.random_scene(SEED).finalize(SEED))
    rs = rt.RenderSettings(samples=mx, seed=SEED, sample_chunk=b)
    accum, counts, moments, _, _ = gpu.render_adaptive(
        cam, rs, rt.AdaptiveSettings(threshold=thr, min_samples=mn, step=step, noise_floor=floor))
    assert len(np.unique(counts)) > 1
    albedo, normal, depth = gpu.render_features(
        cam, rt.RenderSettings(samples=mx, seed=SEED, sample_begin=0, sample_count=mn), chain=8)
    filtered = rt.denoise(accum, albedo, normal, depth, feature_samples=mn, counts=counts,
                          variance=rt.moments_variance(moments, counts, b),
                          settings=rt.DenoiseSettings(iterations=3))
    assert np.array_equal(np.asarray(Image.open(out)), rt.to_image_counts(filtered, counts))


def test_cli_refuses_denoise_where_it_does_not_apply(tmp_path):
    out = str(tmp_path / "x.png")
    r = run_cli("random", "-w", "32", "-s", "4", "--gpus", "2", "--denoise", "3", "-o", out)
    assert r.returncode != 0 and "--denoise" in r.stderr and "one GPU" in r.stderr
    r = run_cli("final", "-w", "32", "-s", "4", "--denoise", "-o", out)
    assert r.returncode != 0 and "--denoise" in r.stderr and "book-2" in r.stderr
    r = run_cli("random", "-w", "32", "-s", "4", "--denoise-variance", "--denoise", "-o", out)
    assert r.returncode != 0 and "--adaptive" in r.stderr
    assert not os.path.exists(out)
