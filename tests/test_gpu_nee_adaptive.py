"""rt_render_nee_adaptive (nee_adaptive.hip, nee_kernel.h; include/shirley_rt.h) against the
restatement of its definition (tests/nee_adaptive_ref.py): the schedule, the sums, the moments and the tile error
over batch frames that come from the CPU oracle's rt_render_nee (tests/nee_ref.py) or, for the scene settings the
oracle does not restate here, from the device's own rt_render_nee range calls.  accum, counts and m1 are compared
exactly; m2 and tile_error within rtol 1e-9 (tests/test_gpu_adaptive.py's figure)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import direct_ref as D
import nee_adaptive_ref as A
import nee_ref as R
import oracle_lib as O
import raytracer as rt
from raytracer import _native as N

pytestmark = pytest.mark.gpu
SEED = 0x5EED
W, H = 28, 20  # 4 x 3 tiles: the last tile column holds 4 pixel columns, the last tile row 4 pixel rows
DEPTH, B, MIN, STEP, MAX, FLOOR, THR = 4, 2, 4, 2, 12, 0.01, 0.6
MIS = [False, True]
INF = float("inf")
CLI = os.path.join(N.BIN_DIR, "ray-cli")


def settings(samples=MAX, depth=DEPTH, b=B, **kw):
    return rt.RenderSettings(samples=samples, max_reflect=depth, seed=SEED, sample_chunk=b, **kw)


def adaptive(thr=THR, mn=MIN, step=STEP, floor=FLOOR):
    return rt.AdaptiveSettings(threshold=thr, min_samples=mn, step=step, noise_floor=floor)


def equal_outputs(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:4], b[:4]))


@pytest.fixture(scope="module")
def hand():
    sc = D.hand_scene(extras=True).finalize(SEED)
    return sc, O.OracleScene(sc)


@pytest.fixture(scope="module")
def main_ref(hand):
    """The main case, computed once on the CPU and left unchanged: the six batch frames of the hand-built scene at
    28x20, MIS clear and set, and their restatement at threshold 0.6."""
    sc, osc = hand
    cam = D.hand_camera(W, H)
    out = {}
    for mis in MIS:
        batches = A.oracle_batches(sc, cam, SEED, B, MAX // B, DEPTH, mis, osc)
        out[mis] = (batches, A.restate(batches, B, MIN, STEP, MAX, FLOOR, THR))
    return out


# ---- 1. the main case ------------------------------------------------------------------------------------

@pytest.mark.parametrize("mis", MIS)
def test_main_case_equals_the_restatement(gpu, hand, main_ref, mis):
    """Every count of the schedule occurs, three tiles are all sky (E = 0: they stop at min_samples), and one tile
    stops at 6 although its error would rise above the threshold again later."""
    sc, _ = hand
    gpu.upload(sc)
    _, ref = main_ref[mis]
    got = gpu.render_nee_adaptive(D.hand_camera(W, H), settings(), adaptive(), mis=mis)
    near = A.compare(got, ref, THR, f"hand {W}x{H} mis {mis}")
    assert near == []  # (the chosen inputs leave no tile out)
    accum, counts, moments, tile_error, rep = got
    tiles = counts[::8, ::8]
    assert np.array_equal(np.kron(tiles, np.ones((8, 8), int))[:H, :W], counts)
    assert len(set(tiles.reshape(-1).tolist())) >= 4
    assert int((tile_error == 0.0).sum()) == 3 and (tiles[tile_error == 0.0] == MIN).all()
    # decisions: a tile that stopped early is at or below the threshold; one that went on to the end was above it
    # at every earlier check
    assert (tile_error[tiles < MAX] <= THR).all()
    assert all(e > THR for t, n, e in ref.checks if n < ref.counts[::8, ::8].reshape(-1)[t])
    later = [e for t, n, e in A.restate(main_ref[mis][0], B, MIN, STEP, MAX, FLOOR, 0.0).checks if t == 3 and n > 6]
    assert tiles.reshape(-1)[3] == 6 and max(later) > THR
    assert rep.tiles == 12 and rep.samples == counts.sum() and rep.steps == 1 + (MAX - MIN) // STEP
    assert rep.tiles_converged == int((tile_error <= THR).sum()) and rep.segments == 0 and rep.fold_ms == 0.0
    assert rep.kernel_ms > 0.0


@pytest.mark.parametrize("thr", [0.5, 0.9])
def test_other_thresholds_give_other_mixes(gpu, hand, main_ref, thr):
    sc, _ = hand
    gpu.upload(sc)
    for mis in MIS:
        ref = A.restate(main_ref[mis][0], B, MIN, STEP, MAX, FLOOR, thr)
        assert not np.array_equal(ref.counts, main_ref[mis][1].counts)
        got = gpu.render_nee_adaptive(D.hand_camera(W, H), settings(), adaptive(thr), mis=mis)
        assert A.compare(got, ref, thr, f"hand {W}x{H} threshold {thr} mis {mis}") == []


# ---- 2. thresholds 0 and +inf, max_depth 0 ---------------------------------------------------------------

@pytest.mark.parametrize("mis", MIS)
def test_threshold_zero_and_infinity(gpu, hand, main_ref, mis):
    sc, _ = hand
    gpu.upload(sc)
    cam = D.hand_camera(W, H)
    batches, _ = main_ref[mis]
    accum, counts, moments, tile_error, rep = got = gpu.render_nee_adaptive(cam, settings(), adaptive(0.0), mis=mis)
    total = np.zeros_like(batches[0])
    for bk in batches:
        total = total + bk
    assert (counts == MAX).all() and np.array_equal(accum, total)
    assert A.compare(got, A.restate(batches, B, MIN, STEP, MAX, FLOOR, 0.0), 0.0, f"threshold 0 mis {mis}") == []
    assert rep.samples == W * H * MAX and rep.steps == 1 + (MAX - MIN) // STEP
    # (a threshold-0 frame is rt_render_nee's up to the grouping of the additions: batch sums, then their sum)
    accum, counts, moments, tile_error, rep = got = gpu.render_nee_adaptive(cam, settings(), adaptive(INF), mis=mis)
    assert (counts == MIN).all() and np.isfinite(tile_error).all() and rep.steps == 1 and rep.tiles_converged == 12
    assert np.array_equal(accum, batches[0] + batches[1])
    assert A.compare(got, A.restate(batches, B, MIN, STEP, MAX, FLOOR, INF), INF, f"threshold inf mis {mis}") == []


def test_max_depth_zero_traces_nothing(gpu, hand):
    sc, _ = hand
    gpu.upload(sc)
    accum, counts, moments, tile_error, rep = gpu.render_nee_adaptive(D.hand_camera(W, H), settings(depth=0),
                                                                      adaptive(0.0))
    assert not accum.any() and not moments.any() and (counts == MIN).all() and not tile_error.any()
    assert rep.steps == 1 and rep.samples == W * H * MIN and rep.tiles_converged == 12


# ---- 3. the grid size and the placements -----------------------------------------------------------------

@pytest.mark.parametrize("nodes,bvh", [("global", "reference"), ("lds", "reference"), ("half-lds", "reference"),
                                       ("auto", "reference"), ("global", "sah"), ("auto", "sah")])
def test_grid_size_placement_and_builder_leave_the_frame_alone(gpu, hand, main_ref, monkeypatch, nodes, bvh):
    """SHIRLEY_NEE_BLOCKS = 1 (a narrow block: four waves serve the twelve tiles, so every wave fetches more than
    once), 2 and unset: every output is bit-identical, and equal to the restatement's."""
    sc, _ = hand
    gpu.upload(sc, bvh=bvh, nodes=nodes)
    cam = D.hand_camera(W, H)
    try:
        for mis in MIS:
            frames = []
            for blocks in ("1", "2", None):
                if blocks is None:
                    monkeypatch.delenv("SHIRLEY_NEE_BLOCKS", raising=False)
                else:
                    monkeypatch.setenv("SHIRLEY_NEE_BLOCKS", blocks)
                frames.append(gpu.render_nee_adaptive(cam, settings(), adaptive(), mis=mis))
            assert equal_outputs(frames[0], frames[1]) and equal_outputs(frames[0], frames[2]), (nodes, bvh, mis)
            assert A.compare(frames[0], main_ref[mis][1], THR, f"{nodes} {bvh} mis {mis}") == []
    finally:
        monkeypatch.delenv("SHIRLEY_NEE_BLOCKS", raising=False)
        gpu.upload(sc)


# ---- 4. small shapes -------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(1, 1), (9, 9), (8, 8)])
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("mis", MIS)
def test_small_shapes(gpu, hand, mis, b, w, h):
    """One live lane in 64 (1x1), four tiles of which three are mostly empty (9x9), one full tile (8x8); a batch of
    one sample (every sample flushes) and of two."""
    sc, osc = hand
    cam = D.hand_camera(w, h)
    gpu.upload(sc)
    mn, step, mx = 2 * b, b, 6 * b
    batches = A.oracle_batches(sc, cam, SEED, b, mx // b, DEPTH, mis, osc)
    for thr in (0.0, THR):
        ref = A.restate(batches, b, mn, step, mx, FLOOR, thr)
        got = gpu.render_nee_adaptive(cam, settings(mx, b=b), adaptive(thr, mn, step), mis=mis)
        assert A.compare(got, ref, thr, f"hand {w}x{h} b {b} threshold {thr} mis {mis}") == []
    assert batches[0].max() > 0.0


# ---- 5. the scene's settings -----------------------------------------------------------------------------

def check_against_device_batches(gpu, cam, depth, mis, label, thresholds):
    """A threshold-0 frame is the batch-order sum of the device's own rt_render_nee range calls; a mixed frame's
    pixels hold the prefix of those sums that `counts` selects (the restatement over those batch frames)."""
    batches = A.device_batches(gpu, cam, lambda **kw: settings(MAX, depth, **kw), B, MAX // B, mis)
    for thr in thresholds:
        ref = A.restate(batches, B, MIN, STEP, MAX, FLOOR, thr)
        got = gpu.render_nee_adaptive(cam, settings(MAX, depth), adaptive(thr), mis=mis)
        assert A.compare(got, ref, thr, f"{label} threshold {thr} mis {mis}") == []
        if thr == 0.0:
            assert (got[1] == MAX).all()
    return batches


@pytest.mark.parametrize("cells", [0, 4])
@pytest.mark.parametrize("mode", [N.RT_LIGHT_SAMPLE_AREA, N.RT_LIGHT_SAMPLE_SOLID_ANGLE,
                                  N.RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL])
@pytest.mark.parametrize("mis", MIS)
def test_light_pick_and_sampling_mode_apply(gpu, hand, mis, mode, cells):
    sc, _ = hand
    gpu.upload(sc)
    try:
        gpu.light_pick(cells)
        gpu.light_sampling(mode)
        cam = D.hand_camera(20, 12)
        plain = check_against_device_batches(gpu, cam, DEPTH, mis, f"hand 20x12 cells {cells} mode {mode}", (0.0, THR))
    finally:
        gpu.upload(sc)  # (the settings last until the next upload)
    if cells or mode != N.RT_LIGHT_SAMPLE_AREA:
        assert not np.array_equal(plain[0], gpu.render_nee(cam, settings(MAX, sample_begin=0, sample_count=B), mis=mis))


def test_light_visibility_applies(gpu, hand):
    sc, _ = hand
    gpu.upload(sc)
    try:
        gpu.light_pick(4)
        gpu.light_visibility(8, SEED)
        check_against_device_batches(gpu, D.hand_camera(20, 12), DEPTH, True, "hand 20x12 visibility K 8", (0.0, THR))
    finally:
        gpu.upload(sc)


@pytest.mark.parametrize("mis", MIS)
def test_cornell(gpu, mis):
    gpu.upload(rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED))
    check_against_device_batches(gpu, rt.cornell_camera(24), 6, mis, "cornell 24x24 depth 6", (0.0, 0.3))


# ---- 6. the device form ----------------------------------------------------------------------------------

def test_device_form_equals_the_host_form_and_feeds_the_consumers(gpu, hand, main_ref):
    import torch
    sc, _ = hand
    cam = D.hand_camera(W, H)
    gpu.upload(sc)
    host = gpu.render_nee_adaptive(cam, settings(), adaptive(), mis=True)
    assert A.compare(host, main_ref[True][1], THR, "host form") == []
    accum = torch.full((H, W, 3), -1.0, dtype=torch.float64, device="cuda")
    moments = torch.full((H, W, 2), -1.0, dtype=torch.float64, device="cuda")
    counts = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    terr = torch.full((3, 4), -1.0, dtype=torch.float64, device="cuda")
    var = torch.zeros((H, W), dtype=torch.float64, device="cuda")
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    gpu.render_nee_adaptive_device(cam, settings(), adaptive(), True, accum.data_ptr(), counts.data_ptr(),
                                   moments.data_ptr(), terr.data_ptr(), stream)
    gpu.moments_variance_device(moments.data_ptr(), counts.data_ptr(), B, W, H, var.data_ptr(), stream)
    gpu.tonemap_counts_device(accum.data_ptr(), counts.data_ptr(), W, H, rgb.data_ptr(), stream)
    torch.cuda.synchronize()
    dev = (accum.cpu().numpy(), counts.cpu().numpy(), moments.cpu().numpy(), terr.cpu().numpy())
    assert equal_outputs(dev, host)  # (so every in-image element was overwritten: the host form's hold no -1)
    assert np.array_equal(var.cpu().numpy(), rt.moments_variance(host[2], host[1], B))
    assert np.array_equal(rgb.cpu().numpy(), rt.to_image_counts(host[0], host[1]))
    # without the errors
    accum.fill_(-1.0)
    torch.cuda.synchronize()
    gpu.render_nee_adaptive_device(cam, settings(), adaptive(), True, accum.data_ptr(), counts.data_ptr(),
                                   moments.data_ptr(), 0, stream)
    torch.cuda.synchronize()
    assert np.array_equal(accum.cpu().numpy(), host[0])


# ---- 7. status codes -------------------------------------------------------------------------------------

def test_status_codes(gpu, hand):
    sc, _ = hand
    cam = D.hand_camera(20, 12)
    lib = N.rt_lib()
    buf = [np.zeros((12, 20, 3)), np.zeros((12, 20), dtype=np.int32), np.zeros((12, 20, 2)), np.zeros((2, 3))]
    ptr = [x.ctypes.data for x in buf]

    def call(p, a, flags=1, ptrs=ptr, device=False):
        if device:
            return lib.rt_render_nee_adaptive_device(gpu.handle, C.byref(cam), C.byref(p), flags, C.byref(a), *ptrs, None)
        return lib.rt_render_nee_adaptive(gpu.handle, C.byref(cam), C.byref(p), flags, C.byref(a), *ptrs, None)

    gpu.upload(rt.scenes.final_scene(SEED, 4, 30).finalize(SEED))
    assert call(settings().params(), adaptive().params()) == N.RT_E_UNSUPPORTED
    gpu.upload(sc)
    p, a = settings().params(), adaptive().params()
    assert call(p, a) == N.RT_OK
    for flags in (2, 3, -1, 1 << 16):
        assert call(p, a, flags) == N.RT_E_INVALID
    assert call(p, a, ptrs=[None] + ptr[1:]) == N.RT_E_INVALID
    assert call(p, a, ptrs=[ptr[0], None] + ptr[2:]) == N.RT_E_INVALID
    assert call(p, a, ptrs=ptr[:2] + [None, None]) == N.RT_OK  # moments and errors may be NULL in the host form
    for k in range(3):  # the device form needs accum, counts and moments (the checks come before any use)
        assert call(p, a, ptrs=[None if i == k else 8 for i in range(3)] + [None], device=True) == N.RT_E_INVALID
    # every adaptive_validate failure
    bad = [(dict(b=-1), {}), (dict(sample_begin=2, sample_count=2), {}), (dict(tile_world=2), {}),
           (dict(tile_world=2, tile_rank=1), {}), (dict(samples=0), {}), (dict(samples=11), {}), ({}, dict(mn=2)),
           ({}, dict(mn=5)), ({}, dict(mn=14)), ({}, dict(step=0)), ({}, dict(step=3)), ({}, dict(thr=-1.0)),
           ({}, dict(thr=float("nan"))), ({}, dict(floor=-0.5)), ({}, dict(floor=INF)), ({}, dict(floor=float("nan")))]
    for skw, akw in bad:
        assert call(settings(**skw).params(), adaptive(**akw).params()) == N.RT_E_INVALID, (skw, akw)
    # rt_render_nee after an adaptive call is what it was
    for mis in MIS:
        ref = R.oracle_nee(sc, cam, SEED, 0, 4, 4, mis, hand[1], stats=False)
        assert np.array_equal(gpu.render_nee(cam, rt.RenderSettings(samples=4, max_reflect=4, seed=SEED), mis=mis),
                              ref.sums)


# ---- 8. ray-cli ------------------------------------------------------------------------------------------

def test_cli_writes_the_picture_and_the_report_line(tmp_path):
    out = tmp_path / "nee_adaptive.png"
    r = subprocess.run([CLI, "render", "cornell", "-w", "64", "-s", "16", "-m", "6", "--seed", "24301", "-v",
                        "--nee", "--nee-adaptive", "0.3", "--min-samples", "8", "--adaptive-step", "4",
                        "--sample-chunk", "4", "-o", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert out.exists() and out.stat().st_size > 0
    assert "INFO adaptive:" in r.stderr and "of 64 tiles converged" in r.stderr
