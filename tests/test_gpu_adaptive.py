"""Adaptive sampling on the GPU (ABI 8: rt_render_adaptive, rt_tonemap_counts*).

One setup for every case: random_scene, a 44x28 frame (6x4 tiles with a partial tile column and a partial
tile row), batch 4, min_samples 8, step 8, at most 32 samples.  The counter RNG is keyed by the global
(pixel, sample) and the fold continues each pixel's chunk-order sum, so a pixel that stopped after n
samples must equal rt_render's sample range [0, n) with the same sample_chunk bit for bit.
"""
import numpy as np
import pytest

import oracle_lib as O
import raytracer as rt
from raytracer import _native as N

pytestmark = pytest.mark.gpu

SEED = 0x5EED
W, H, TX, TY = 44, 28, 6, 4
B, MIN, STEP, MAX = 4, 8, 8, 32
FLOOR = 0.01
INF = float("inf")
BASE = dict(samples=MAX, seed=SEED, sample_chunk=B)


def camera():
    # default_camera's position and lens (scenes.rs:214-231) on a 44x28 frame
    cam = rt.CameraBuilder(width=W, aspect_ratio=(11, 7), vfov=20.0, focal_length=1.0, aperture=0.001).build(
        rt.CameraPosition((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), focus_length=10.0))
    assert (cam.image_width, cam.image_height) == (W, H)
    return cam


def adaptive(threshold, **kw):
    return rt.AdaptiveSettings(**{**dict(threshold=threshold, min_samples=MIN, step=STEP, noise_floor=FLOOR), **kw})


@pytest.fixture(scope="module")
def scene():
    return rt.scenes.random_scene(SEED).finalize(SEED)


@pytest.fixture(scope="module")
def shared(gpu, scene):
    """Computed once: the uniform frames of sample ranges [0, n) (the references of every case) and the
    adaptive run that stops every tile at min_samples (its tile errors calibrate the thresholds)."""
    cam = camera()
    gpu.upload(scene)
    ref = {n: gpu.render(cam, rt.RenderSettings(**BASE, sample_count=n)) for n in range(MIN, MAX + 1, STEP)}
    assert np.array_equal(ref[MAX], gpu.render(cam, rt.RenderSettings(**BASE)))
    for r in ref.values():
        r.setflags(write=False)
    at_min = gpu.render_adaptive(cam, rt.RenderSettings(**BASE), adaptive(INF))
    return dict(cam=cam, ref=ref, at_min=at_min)


def tile_index_image():
    """[H][W]: the index of each pixel's 8x8 tile (tile k = (k % TX, k // TX), row 0 = bottom)."""
    jj, ii = np.mgrid[0:H, 0:W]
    return (jj // 8) * TX + ii // 8


def errors_from_moments(moments, counts, floor=FLOOR):
    """The tile error formula of shirley_rt.h in numpy, from the returned moments and counts."""
    tid = tile_index_image()
    e = np.zeros(TX * TY)
    for t in range(TX * TY):
        m = tid == t
        n_samples = counts[m]
        assert (n_samples == n_samples[0]).all()
        n, K = int(n_samples[0]) // B, int(m.sum())
        m1, m2 = moments[m][:, 0], moments[m][:, 1]
        v = np.maximum(0.0, m2 - m1 * m1 / n) / (n - 1)
        e[t] = np.sqrt(n * v.sum() / K) / (m1.sum() / K + n * B * floor)
    return e.reshape(TY, TX)


def check_adaptive(gpu, shared, thr, max_samples=MAX):
    """The checks of a frame whose tiles stopped at different counts; returns (counts, tile_error)."""
    cam, ref = shared["cam"], shared["ref"]
    accum, counts, moments, tile_error, rep = gpu.render_adaptive(
        cam, rt.RenderSettings(**{**BASE, "samples": max_samples}), adaptive(thr))
    # every pixel holds exactly its own samples [0, n) of the uniform frame
    present = sorted(set(counts.reshape(-1).tolist()))
    assert set(present) <= set(range(MIN, max_samples + 1, STEP))
    for n in present:
        assert np.array_equal(accum[counts == n], ref[n][counts == n]), f"pixels with {n} samples"
    tile_counts = counts[::8, ::8]
    assert tile_counts.shape == (TY, TX) and np.array_equal(np.kron(tile_counts, np.ones((8, 8), int))[:H, :W], counts)
    assert rep.samples == counts.sum() and rep.tiles == TX * TY and rep.steps == (present[-1] - MIN) // STEP + 1
    # the error the device computed is the documented formula of the returned moments
    e = errors_from_moments(moments, counts)
    print("tile errors", tile_error.round(6).tolist(), "threshold", thr, "counts", tile_counts.tolist())
    assert np.allclose(tile_error, e, rtol=1e-9, atol=0)
    # decisions: a tile that stopped early is below the threshold (tiles on the threshold are left out)
    near = np.abs(tile_error - thr) <= 1e-9 * thr
    assert near.sum() == 0  # (the seed leaves none out; at most 1 % would be allowed)
    stopped = (tile_counts < max_samples) & ~near
    assert (tile_error[stopped] <= thr).all()
    assert rep.tiles_converged == int((tile_error <= thr).sum())
    return counts, tile_error


# ---- threshold 0: every tile reaches the maximum through the list path --------------------------------

def full_list_case(gpu, scene, cam, ref, bvh_nodes):
    gpu.upload(scene, nodes=bvh_nodes)
    for scratch in (0, 1):
        s = rt.RenderSettings(**{**BASE, "scratch_mb": scratch})
        accum, counts, _, tile_error, rep = gpu.render_adaptive(cam, s, adaptive(0.0))
        assert np.array_equal(accum, ref)
        assert (counts == MAX).all() and rep.samples == counts.sum() == cam.image_width * cam.image_height * MAX
        assert rep.steps == (MAX - MIN) // STEP + 1 and rep.segments > rep.samples
        assert np.isfinite(tile_error).all() and (tile_error >= 0).all() and rep.tiles_converged == 0


@pytest.mark.parametrize("nodes", ["auto", "global"])
def test_threshold_zero_equals_uniform_frame(gpu, scene, shared, nodes):
    """nodes=auto: the scene-in-LDS block; nodes=global: the 256-thread instances.  (A step's partials are
    73 KB here, one pass under any bound: test_scratch_bound_splits_a_step_into_passes has the frame that
    scratch_mb=1 splits.)"""
    full_list_case(gpu, scene, shared["cam"], shared["ref"][MAX], nodes)


def test_threshold_zero_book2_scene(gpu):
    """The EXT kernel instances: a small final_scene (moving spheres, media, instances), 44x44."""
    scene = rt.scenes.final_scene(SEED, 4, 30).finalize(SEED)
    cam = rt.scene_camera("final", 44, "square")
    gpu.upload(scene)
    ref = gpu.render(cam, rt.RenderSettings(**BASE))
    full_list_case(gpu, scene, cam, ref, "auto")


def test_scratch_bound_splits_a_step_into_passes(gpu, scene, monkeypatch):
    """A 1 MiB bound on a 200x133 frame (25x17 tiles: 653 KB of partials per chunk) renders a 2-chunk step
    over every tile in 2 passes: the frame, the moments and the errors are bit-identical to the unbounded
    call's, for the full lists (threshold 0) and for mixed ones, and so are they when the device refuses the
    partial buffer (simulated) and the step falls back to smaller passes."""
    cam = rt.default_camera(200, "std3x2")
    assert ((cam.image_width + 7) // 8) * ((cam.image_height + 7) // 8) * 64 * 24 * 2 > (1 << 20)
    gpu.upload(scene)
    s = dict(samples=16, seed=SEED, sample_chunk=B)
    at_min = gpu.render_adaptive(cam, rt.RenderSettings(**s), adaptive(INF))
    for thr in (0.0, float(np.median(at_min[3]))):
        one = gpu.render_adaptive(cam, rt.RenderSettings(**s), adaptive(thr))
        assert gpu.counters().passes == 1
        two = gpu.render_adaptive(cam, rt.RenderSettings(**s, scratch_mb=1), adaptive(thr))
        assert thr > 0 or gpu.counters().passes == 2
        monkeypatch.setenv("SHIRLEY_SIMULATE_OOM_MB", "1")
        oom = gpu.render_adaptive(cam, rt.RenderSettings(**s), adaptive(thr))
        monkeypatch.delenv("SHIRLEY_SIMULATE_OOM_MB")
        for other in (two, oom):
            for a, b in zip(one[:4], other[:4]):
                assert np.array_equal(a, b)
            assert one[4].samples == other[4].samples and one[4].segments == other[4].segments
        assert len(np.unique(one[1])) == (1 if thr == 0 else 2)
        assert np.array_equal(one[0][one[1] == 16], gpu.render(cam, rt.RenderSettings(**s))[one[1] == 16])


# ---- threshold inf: every tile stops at min_samples ---------------------------------------------------

def test_threshold_inf_stops_at_min_samples(shared):
    accum, counts, moments, tile_error, rep = shared["at_min"]
    assert (counts == MIN).all() and np.array_equal(accum, shared["ref"][MIN])
    assert rep.steps == 1 and rep.samples == W * H * MIN and rep.tiles_converged == rep.tiles == TX * TY
    assert np.allclose(tile_error, errors_from_moments(moments, counts), rtol=1e-9, atol=0)


# ---- mixed lists ----------------------------------------------------------------------------------------

def test_mixed_thresholds(gpu, scene, shared):
    """The median of the tile errors at min_samples as the threshold: about half the tiles go on."""
    gpu.upload(scene)
    thr = float(np.median(shared["at_min"][3]))
    counts, tile_error = check_adaptive(gpu, shared, thr)
    tile_counts = counts[::8, ::8]
    assert (tile_counts > MIN).sum() == TX * TY // 2  # (the tiles strictly above the median)
    # the tiles with the largest count were still above the threshold one step earlier
    n = int(tile_counts.max())
    assert n > MIN
    _, tile_error_before = check_adaptive(gpu, shared, thr, max_samples=n - STEP)
    went_on = tile_counts == n
    near = np.abs(tile_error_before - thr) <= 1e-9 * thr
    assert went_on.any() and (tile_error_before[went_on & ~near] > thr).all()


def test_single_tile_list(gpu, scene, shared):
    """A threshold between the two largest tile errors: the second step's list is one tile (64 units per
    chunk, fewer than one block takes)."""
    gpu.upload(scene)
    e = np.sort(shared["at_min"][3].reshape(-1))
    assert e[-1] > e[-2]
    thr = float(0.5 * (e[-1] + e[-2]))
    counts, tile_error = check_adaptive(gpu, shared, thr)
    tile_counts = counts[::8, ::8]
    assert (tile_counts > MIN).sum() == 1 and tile_counts[np.unravel_index(np.argmax(shared["at_min"][3]), (TY, TX))] > MIN


# ---- moments against the oracle -------------------------------------------------------------------------

def test_moments_match_oracle(gpu, scene, shared):
    """m1, m2 of 16 pixels (interior tiles, the partial tile column x >= 40 and the partial tile row y >= 24)
    from the oracle's per-sample colours: batch sums of 4 in order, y = (r + g) + b.  Tolerances: the
    module tolerance of test_gpu_parity.py for sums (1e-10 per sample, absolute) on m1, twice that on m2."""
    cam = shared["cam"]
    gpu.upload(scene)
    accum, counts, moments, _, _ = gpu.render_adaptive(cam, rt.RenderSettings(**BASE), adaptive(0.0))
    ora = O.OracleScene(scene)
    p = O.params(MAX, 50, SEED)
    tol = 1e-10 * MAX
    for px in (3, 13, 30, 43):
        for py in (2, 11, 20, 27):
            m1 = m2 = 0.0
            total = np.zeros(3)
            for c in range(MAX // B):
                batch = np.zeros(3)
                for s in range(c * B, (c + 1) * B):
                    batch = batch + ora.sample(cam, p, px, py, s)[0]
                total = total + batch
                y = (batch[0] + batch[1]) + batch[2]
                m1 += y
                m2 += y * y
            print(f"pixel ({px}, {py}): m1 {float(moments[py, px, 0])!r} oracle {float(m1)!r}, m2 {float(moments[py, px, 1])!r} oracle {float(m2)!r}")
            assert np.all(np.abs(accum[py, px] - total) <= tol)
            assert abs(moments[py, px, 0] - m1) <= tol
            assert abs(moments[py, px, 1] - m2) <= 2 * tol


# ---- refused calls ----------------------------------------------------------------------------------------

def test_invalid_arguments_and_unsupported_engines(gpu, scene, shared):
    cam = shared["cam"]
    gpu.upload(scene)

    def status(settings=None, **ad):
        with pytest.raises(rt.RtError) as err:
            gpu.render_adaptive(cam, rt.RenderSettings(**{**BASE, **(settings or {})}), adaptive(0.05, **ad))
        return err.value.code

    assert status(step=6) == N.RT_E_INVALID                          # not a multiple of the batch
    assert status(min_samples=4) == N.RT_E_INVALID                   # fewer than 2 batches
    assert status(dict(sample_begin=4)) == N.RT_E_INVALID
    assert status(dict(sample_count=8)) == N.RT_E_INVALID
    assert status(dict(tile_world=2)) == N.RT_E_INVALID
    assert status(dict(samples=30)) == N.RT_E_INVALID
    assert status(noise_floor=-1.0) == N.RT_E_INVALID
    assert status(dict(engine="wavefront")) == N.RT_E_UNSUPPORTED
    assert status(dict(engine="split")) == N.RT_E_UNSUPPORTED
    assert "megakernel" in N.rt_lib().rt_last_error(gpu.handle).decode()
    # the context still renders, explicitly on the megakernel too
    accum, counts, *_ = gpu.render_adaptive(cam, rt.RenderSettings(**BASE, engine="megakernel"), adaptive(INF))
    assert np.array_equal(accum, shared["ref"][MIN])


def test_max_depth_zero_is_black_and_stops(gpu, scene, shared):
    gpu.upload(scene)
    accum, counts, moments, tile_error, rep = gpu.render_adaptive(
        shared["cam"], rt.RenderSettings(**BASE, max_reflect=0), adaptive(0.05, noise_floor=0.0))
    assert not accum.any() and not moments.any() and (counts == MIN).all() and not tile_error.any()
    assert rep.steps == 1 and rep.tiles_converged == TX * TY and rep.samples == W * H * MIN


# ---- tonemap ------------------------------------------------------------------------------------------------

def test_tonemap_counts(gpu, scene, shared):
    """rt_tonemap_counts_device == rt_tonemap_counts byte for byte on a mixed frame (with NaN, zero-count and
    saturating pixels planted); uniform counts give rt_tonemap's bytes on both."""
    import torch
    gpu.upload(scene)
    thr = float(np.median(shared["at_min"][3]))
    accum, counts, *_ = gpu.render_adaptive(shared["cam"], rt.RenderSettings(**BASE), adaptive(thr))
    assert len(np.unique(counts)) > 1
    accum, counts = accum.copy(), counts.copy()
    accum[0, 0] = np.nan
    accum[1, 1] = 1e9
    accum[2, 2] = -1.0
    counts[3, 3] = 0
    counts[4, 4] = -5

    def on_device(a, n):
        da, dn = torch.from_numpy(np.ascontiguousarray(a)).to("cuda"), torch.from_numpy(np.ascontiguousarray(n)).to("cuda")
        out = torch.full(a.shape, 77, dtype=torch.uint8, device="cuda")
        gpu.tonemap_counts_device(da.data_ptr(), dn.data_ptr(), a.shape[1], a.shape[0], out.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    host = rt.to_image_counts(accum, counts)
    assert np.array_equal(on_device(accum, counts), host)
    assert not host[H - 1 - 3, 3].any() and not host[H - 1 - 4, 4].any() and not host[H - 1, 0].any()
    assert (host[H - 1 - 1, 1] == 255).all()
    # each pixel is divided by its own count
    j, i = np.argwhere(counts == counts.max())[0]
    assert np.array_equal(host[H - 1 - j, i], rt.to_image(accum[j:j + 1, i:i + 1], int(counts[j, i]))[0, 0])
    for n in (MIN, MAX, 1):
        uniform = np.full((H, W), n, dtype=np.int32)
        want = rt.to_image(accum, n)
        assert np.array_equal(rt.to_image_counts(accum, uniform), want)
        assert np.array_equal(on_device(accum, uniform), want)


# ---- ray-cli ------------------------------------------------------------------------------------------------

def test_cli_adaptive_picture_and_report(gpu, tmp_path):
    """`ray-cli render random --adaptive T`: the PNG is the counts tonemap of the library's adaptive frame,
    and -v prints the steps, the mean spp and the converged share."""
    import os
    import re
    import subprocess
    from PIL import Image
    cli = os.path.join(N.BIN_DIR, "ray-cli")
    out = str(tmp_path / "adaptive.png")
    r = subprocess.run([cli, "-v", "render", "random", "-w", "96", "-s", str(MAX), "--seed", hex(SEED),
                        "--camera-aspect-ratio", "std16x9", "--sample-chunk", str(B), "--adaptive", "0.2",
                        "--min-samples", str(MIN), "--adaptive-step", str(STEP), "--noise-floor", str(FLOOR), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cam = rt.scene_camera("random", 96, "std16x9")
    gpu.upload(rt.scenes.random_scene(SEED).finalize(SEED))
    accum, counts, _, _, rep = gpu.render_adaptive(cam, rt.RenderSettings(**BASE), adaptive(0.2))
    assert len(np.unique(counts)) > 1
    assert np.array_equal(np.asarray(Image.open(out)), rt.to_image_counts(accum, counts))
    m = re.search(r"INFO adaptive: (\d+) steps, mean ([\d.]+) spp of at most (\d+), ([\d.]+) % of (\d+) tiles converged",
                  r.stderr)
    assert m, r.stderr
    assert (int(m[1]), int(m[3]), int(m[5])) == (rep.steps, MAX, rep.tiles)
    assert abs(float(m[2]) - counts.mean()) <= 0.005 and abs(float(m[4]) - 100.0 * rep.tiles_converged / rep.tiles) <= 0.05
