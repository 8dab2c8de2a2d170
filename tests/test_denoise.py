"""The à-trous filter on the CPU (rt_denoise, csrc/rt/denoise.h; include/shirley_rt.h ABI 10): bit-exact
against a numpy restatement of its definition, its properties (identity, constants, hard edges, NaN and
count-0 pixels, argument rules), its quality on an oracle render of the Cornell box, and the same header as a
stand-alone program built plainly and with AddressSanitizer + UBSan (tools/denoise_check.cpp)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import oracle_lib as O
import raytracer as rt
from raytracer import _native as N

REPO = O.REPO
SEED = 0x5EED


@pytest.fixture(scope="module")
def frames():
    return {(w, h): R.synthetic(w, h) for w, h in R.SIZES}


# ---- bit-exact against numpy ------------------------------------------------------------------------
@pytest.mark.parametrize("use_variance", [False, True])
@pytest.mark.parametrize("use_counts", [False, True])
@pytest.mark.parametrize("iterations", R.ITERATIONS)
@pytest.mark.parametrize("size", R.SIZES)
def test_host_filter_equals_the_numpy_restatement_bit_for_bit(frames, size, iterations, use_counts, use_variance):
    f = frames[size]
    accum, kw = R.case_arrays(f, use_counts, use_variance)
    S = rt.DenoiseSettings(iterations=iterations)
    got = rt.denoise(accum, f["albedo"], f["normal"], f["depth"], settings=S, **kw)
    want = R.numpy_denoise(accum, f["albedo"], f["normal"], f["depth"], settings=S, **kw)
    assert np.all(np.isfinite(got))
    assert R.same_bits(got, want)
    if iterations:
        assert not np.array_equal(got, accum)  # (the filter did something)


# ---- properties -------------------------------------------------------------------------------------
def flat(w, h, samples=16, fs=4, normal=(0.0, 0.0, 1.0), albedo=(0.5, 0.4, 0.3), depth=3.0):
    return dict(albedo=np.tile(np.array(albedo) * fs, (h, w, 1)), normal=np.tile(np.array(normal) * fs, (h, w, 1)),
                depth=np.full((h, w), depth * fs), samples=samples, feature_samples=fs)


def test_zero_iterations_is_the_identity(frames):
    f = frames[(37, 21)]
    for use_counts in (False, True):
        accum, kw = R.case_arrays(f, use_counts, True)
        got = rt.denoise(accum, f["albedo"], f["normal"], f["depth"], settings=rt.DenoiseSettings(iterations=0), **kw)
        assert R.same_bits(got, accum)


@pytest.mark.parametrize("iterations", [1, 8])
def test_constant_demodulated_colour_stays_constant(iterations):
    w, h = 19, 13
    g = flat(w, h)
    rng = np.random.default_rng(3)
    # the albedo varies (within sigma_a), c / a does not: the filter sees a constant image
    g["albedo"] = g["albedo"] * (1.0 + 0.05 * rng.standard_normal((h, w, 1)))
    chat = np.array([0.9, 1.7, 0.25])
    accum = (g["albedo"] / g["feature_samples"]) * chat * g["samples"]
    out = rt.denoise(accum, settings=rt.DenoiseSettings(iterations=iterations), **g)
    # 26 roundings per iteration x up to 8 iterations of 2^-53 each, with margin
    assert np.max(np.abs(out - accum) / accum) <= 1e-13


@pytest.mark.parametrize("feature", ["normal", "albedo", "depth"])
def test_half_planes_do_not_mix(feature):
    w, h = 24, 10
    g = flat(w, h)
    right = np.zeros((h, w), dtype=bool)
    right[:, w // 2:] = True
    if feature == "normal":
        g["normal"][right] = np.array([1.0, 0.0, 0.0]) * g["feature_samples"]      # perpendicular: cos = 0
    elif feature == "albedo":
        g["albedo"][right] = np.array([0.9, 0.1, 0.6]) * g["feature_samples"]      # |da|^2 = 0.34 > sigma_a^2 = 0.04
    else:
        g["depth"][right] = 4.0 * g["feature_samples"]                             # r = 1/7 / 0.05 > 1
    rng = np.random.default_rng(11)
    chat = np.where(right[..., None], 2.0, 0.5) * (1.0 + 0.2 * rng.standard_normal((h, w, 3)))
    A = g["albedo"] / g["feature_samples"]
    accum = chat * A * g["samples"]
    out = rt.denoise(accum, settings=rt.DenoiseSettings(iterations=4), **g)
    # the weight across the edge is exactly 0: each half equals the filter run on that half alone
    for half in (slice(0, w // 2), slice(w // 2, w)):
        sub = {k: (v[:, half] if isinstance(v, np.ndarray) else v) for k, v in g.items()}
        alone = rt.denoise(np.ascontiguousarray(accum[:, half]), settings=rt.DenoiseSettings(iterations=4), **sub)
        assert R.same_bits(out[:, half], alone)
    chat_out = out / (A * g["samples"])
    assert chat_out[:, : w // 2].max() < 1.0 < chat_out[:, w // 2:].min()


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_pixel_passes_through_and_does_not_spread(bad):
    w, h = 17, 11
    g = flat(w, h)
    rng = np.random.default_rng(5)
    accum = np.tile(np.array([4.0, 3.0, 2.0]), (h, w, 1)) * (1.0 + 0.1 * rng.standard_normal((h, w, 3)))
    accum[5, 8, 1] = bad
    S = rt.DenoiseSettings(iterations=3)
    out = rt.denoise(accum, settings=S, **g)
    assert np.array_equal(np.isfinite(out), np.isfinite(accum))
    assert not np.isfinite(out[5, 8, 1])
    # the other pixels: the numpy restatement, which gives the bad pixel weight 0 (and is not its own copy-through)
    want = R.numpy_denoise(accum, g["albedo"], g["normal"], g["depth"], g["samples"], g["feature_samples"], S)
    ok = np.isfinite(accum).all(axis=-1)
    assert R.same_bits(out[ok], want[ok])
    # the bad pixel's finite channels come back as they went in (one division and one product each way)
    assert np.allclose(out[5, 8, [0, 2]], accum[5, 8, [0, 2]], rtol=1e-15)


def test_count_zero_pixels_output_zero_and_are_no_neighbours():
    w, h = 15, 9
    g = flat(w, h)
    del g["samples"]
    rng = np.random.default_rng(9)
    counts = np.full((h, w), 16, dtype=np.int32)
    counts[4, 7] = 0
    counts[0, 0] = 0
    mean = 0.3 * (1.0 + 0.1 * rng.standard_normal((h, w, 3)))
    accum = mean * counts[..., None]
    poisoned = accum.copy()
    poisoned[4, 7] = 1e9          # whatever a count-0 pixel holds is never read as a neighbour
    poisoned[0, 0] = np.nan
    S = rt.DenoiseSettings(iterations=3)
    out = rt.denoise(accum, counts=counts, settings=S, **g)
    out_p = rt.denoise(poisoned, counts=counts, settings=S, **g)
    assert np.all(out[4, 7] == 0.0) and np.all(out[0, 0] == 0.0)
    assert R.same_bits(out, out_p)
    assert np.all(np.isfinite(out))


GOOD = dict(iterations=3, normal_power_log2=4, sigma_z=0.05, sigma_a=0.2, sigma_c=2.0, albedo_floor=1e-3)


def call_raw(w=4, h=4, samples=16, fs=4, counts=None, null=None, out_null=False, **prm):
    g = flat(w, h)
    arrs = dict(accum=np.ones((h, w, 3)), albedo=g["albedo"], normal=g["normal"], depth=g["depth"])
    i = N.rt_denoise_inputs()
    i.width, i.height, i.samples, i.feature_samples = w, h, samples, fs
    for k, v in arrs.items():
        setattr(i, k, None if k == null else v.ctypes.data)
    if counts is not None:
        cn = np.ascontiguousarray(counts, dtype=np.int32)
        i.counts = cn.ctypes.data
    p = rt.DenoiseSettings(**{**GOOD, **prm}).params()
    out = np.zeros((h, w, 3))
    return N.rt_lib().rt_denoise(C.byref(i), C.byref(p), None if out_null else out.ctypes.data)


def test_argument_rules():
    assert call_raw() == N.RT_OK
    assert call_raw(iterations=0) == N.RT_OK and call_raw(iterations=8) == N.RT_OK
    assert call_raw(counts=np.full((4, 4), 3)) == N.RT_OK
    assert call_raw(samples=0, counts=np.zeros((4, 4))) == N.RT_OK      # counts given: `samples` is not read
    bad = [dict(iterations=-1), dict(iterations=9), dict(normal_power_log2=-1), dict(normal_power_log2=17),
           dict(sigma_z=0.0), dict(sigma_a=0.0), dict(sigma_c=0.0), dict(sigma_z=-1.0), dict(sigma_a=float("nan")),
           dict(sigma_c=-2.0), dict(albedo_floor=0.0), dict(albedo_floor=-1e-3), dict(samples=0), dict(samples=-4),
           dict(fs=0), dict(w=0), dict(h=0), dict(null="accum"), dict(null="albedo"), dict(null="normal"),
           dict(null="depth"), dict(out_null=True)]
    for kw in bad:
        assert call_raw(**kw) == N.RT_E_INVALID, kw
    neg = np.full((4, 4), 8)
    neg[2, 1] = -1
    assert call_raw(counts=neg) == N.RT_E_INVALID
    assert N.rt_lib().rt_denoise(None, None, None) == N.RT_E_INVALID


def test_moments_variance_is_the_variance_of_the_mean():
    rng = np.random.default_rng(2)
    h, w, b = 5, 6, 4
    nb = rng.integers(2, 9, size=(h, w))
    counts = (nb * b).astype(np.int32)
    moments = np.zeros((h, w, 2))
    want = np.zeros((h, w))
    for j in range(h):
        for i in range(w):
            y = rng.uniform(0.0, 3.0, nb[j, i]) * b          # batch sums' r+g+b
            moments[j, i] = [y.sum(), (y * y).sum()]
            want[j, i] = y.var(ddof=1) * nb[j, i] / counts[j, i] ** 2   # var(sum of n batches) / N^2
    got = rt.moments_variance(moments, counts, b)
    assert np.allclose(got, want, rtol=1e-9)
    counts[0, 0] = b                                          # one batch: no estimate
    assert np.isnan(rt.moments_variance(moments, counts, b)[0, 0])
    counts[0, 0] = -4
    with pytest.raises(rt.RtError):
        rt.moments_variance(moments, counts, b)


# ---- quality on the oracle --------------------------------------------------------------------------
def oracle_features(scene, osc, cam, seed, spp):
    """First-hit albedo / normal / depth sums from the oracle's camera rays (a scene without dielectrics)."""
    h, w = cam.image_height, cam.image_width
    albedo, normal, depth = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w))
    d, L = scene.desc, O.lib()
    ray, tv = O._d6(), (C.c_double * 3)()
    for py in range(h):
        for px in range(w):
            for s in range(spp):
                L.or_pixel_ray(C.byref(cam), seed, px, py, s, ray)
                hit = osc.hit(ray, index=py * w + px)
                if not hit.hit:
                    continue  # Cornell: the sky is black, normal 0, depth 0
                m = d.materials[d.objects[hit.object].material]
                assert m.kind != N.RT_MAT_DIELECTRIC
                if m.kind == N.RT_MAT_METAL:
                    a = list(m.albedo)
                else:
                    L.or_texture_value(osc.h, m.texture, hit.u, hit.v, hit.point, tv)
                    a = list(tv)
                albedo[py, px] += a
                normal[py, px] += list(hit.normal)
                depth[py, px] += hit.t
    return albedo, normal, depth


def test_cornell_16spp_filtered_error_is_at_most_half_the_noisy_error():
    scene = rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED)
    cam = rt.cornell_camera(48)
    cam.has_lens = 0
    osc = O.OracleScene(scene)
    spp = 16
    noisy, _ = osc.render(cam, O.params(spp, 50, SEED, chunk=spp))
    ref, _ = osc.render(cam, O.params(1024, 50, SEED + 1))
    albedo, normal, depth = oracle_features(scene, osc, cam, SEED, spp)
    out = rt.denoise(noisy, albedo, normal, depth, samples=spp, settings=rt.DenoiseSettings(iterations=3))

    def rmse(x, n):
        return float(np.sqrt(np.mean((np.minimum(x / n, 1.0) - np.minimum(ref / 1024, 1.0)) ** 2)))
    e_noisy, e_filtered = rmse(noisy, spp), rmse(out, spp)
    print(f"cornell 48x48 @ {spp} spp: RMSE noisy {e_noisy:.4f}, filtered {e_filtered:.4f}, "
          f"ratio {e_filtered / e_noisy:.3f}")
    assert e_filtered <= 0.5 * e_noisy


# ---- the header as a stand-alone program, plain and sanitised ----------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("denoise")
    exe = str(d / ("denoise_check_" + request.param))
    flags = ["-O1"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                   ["-o", exe, os.path.join(REPO, "tools", "denoise_check.cpp")], check=True, timeout=180)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True, timeout=60)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return [ln for ln in out.stdout.split("\n") if ln.strip()]
    run.dir = d
    return run


def tool_filter(tool, accum, f, S, kw):
    h, w, _ = accum.shape
    counts, var = kw.get("counts"), kw.get("variance")
    blob = struct.pack("8i4d", w, h, kw["samples"], kw["feature_samples"], counts is not None, var is not None,
                       S.iterations, S.normal_power_log2, S.sigma_z, S.sigma_a, S.sigma_c, S.albedo_floor)
    for a in (accum, f["albedo"], f["normal"], f["depth"]):
        blob += np.ascontiguousarray(a, dtype=np.float64).tobytes()
    if counts is not None:
        blob += np.ascontiguousarray(counts, dtype=np.int32).tobytes()
    if var is not None:
        blob += np.ascontiguousarray(var, dtype=np.float64).tobytes()
    src, dst = str(tool.dir / "in.bin"), str(tool.dir / "out.bin")
    with open(src, "wb") as fh:
        fh.write(blob)
    assert tool("filter", src, dst) == ["ok"]
    return np.fromfile(dst, dtype=np.float64).reshape(h, w, 3)


@pytest.mark.parametrize("iterations", [0, 3, 6])
def test_standalone_filter_equals_the_library(tool, frames, iterations):
    S = rt.DenoiseSettings(iterations=iterations)
    for size in R.SIZES:
        f = frames[size]
        for use_counts, use_variance in ((False, False), (True, True)):
            accum, kw = R.case_arrays(f, use_counts, use_variance)
            accum = accum.copy()
            accum[1, 2, 0] = np.nan     # a copy-through pixel on the way
            got = tool_filter(tool, accum, f, S, kw)
            want = rt.denoise(accum, f["albedo"], f["normal"], f["depth"], settings=S, **kw)
            ok = np.isfinite(want)
            assert np.array_equal(ok, np.isfinite(got)) and R.same_bits(got[ok], want[ok])


def test_standalone_argument_rules(tool):
    good = [4, 4, 16, 4, 0, 3, 4, 0.05, 0.2, 2.0, 1e-3]
    assert tool("validate", *good) == ["ok"]
    for idx, v in ((0, 0), (1, 70000), (2, 0), (3, 0), (5, -1), (5, 9), (6, 17), (7, 0.0), (8, -0.2), (9, "nan"),
                   (10, 0.0)):
        a = list(good)
        a[idx] = v
        assert tool("validate", *a)[0].startswith("invalid "), (idx, v)
    a = list(good)
    a[2], a[4] = 0, 1            # counts given: samples is not read
    assert tool("validate", *a) == ["ok"]
    v = [float(x) for x in tool("variance", 4, "10.0:60.0:8", "1.0:1.0:4", "12.0:50.0:12")]
    assert v[0] == pytest.approx(max(0.0, 60.0 - 100.0 / 2) / 1 * 2 / 64) and np.isnan(v[1])
    assert v[2] == pytest.approx(max(0.0, 50.0 - 144.0 / 3) / 2 * 3 / 144)
