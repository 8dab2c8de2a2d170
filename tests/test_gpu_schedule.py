"""The megakernel's work distribution (trace.hip step 2, csrc/rt/plan.h): however the work units reach the waves —
from the one shared queue in windows of 64, 256 or 1024 units, or from per-block segments with stealing — the frame
and the samples / segments counters of a fixed sample_chunk are the same, bit for bit.

The plan picks the 256-unit window only from 128 units per resident lane (tens of millions of units) and segments
only for units of 4 samples or more, so the call-time switches SHIRLEY_WINDOW and SHIRLEY_SEGMENTS (rt_api.cpp
render_window) force each distribution at test sizes.  Every forced distribution is compared with the default one over
the whole frame, and the default one with the oracle's chunked frame: for chunk c of the range the oracle's frame of
samples [c * chunk, (c + 1) * chunk), added in chunk order — what reduce_kernel adds — by the parity rule of
tests/test_gpu_parity.py.  All on random_scene, on the megakernel.
"""
import contextlib

import numpy as np
import pytest

import oracle_lib as O
import raytracer as rt
from test_gpu_adaptive import BASE as ADAPTIVE_BASE
from test_gpu_adaptive import MAX, MIN, STEP, adaptive, check_adaptive
from test_gpu_adaptive import camera as adaptive_camera
from test_gpu_parity import check_parity

pytestmark = pytest.mark.gpu

SEED = 0x5EED
KEYS = ("SHIRLEY_WINDOW", "SHIRLEY_SEGMENTS")


@pytest.fixture(scope="module")
def scene():
    sc = rt.scenes.random_scene(SEED).finalize(SEED)
    return sc, O.OracleScene(sc)


@pytest.fixture(scope="module")
def cache():
    """Default-distribution frames and chunked oracle frames, computed once and left unchanged."""
    return {}


@pytest.fixture(autouse=True)
def no_switch(monkeypatch):
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)


@contextlib.contextmanager
def switches(monkeypatch, **env):
    """The call-time switches, set around the render calls inside and cleared again."""
    for k, v in env.items():
        monkeypatch.setenv("SHIRLEY_" + k, str(v))
    try:
        yield
    finally:
        for k in env:
            monkeypatch.delenv("SHIRLEY_" + k, raising=False)


def frame_camera(width, height):
    # default_camera's position and lens (scenes.rs:214-231) on a frame of exactly width x height
    cam = rt.CameraBuilder(width=width, aspect_ratio=(width, height), vfov=20.0, focal_length=1.0, aperture=0.001).build(
        rt.CameraPosition((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), focus_length=10.0))
    assert (cam.image_width, cam.image_height) == (width, height)
    return cam


def settings(spp, chunk, **kw):
    return rt.RenderSettings(samples=spp, max_reflect=50, seed=SEED, sample_chunk=chunk, engine="megakernel", **kw)


def n_units(cam, spp, chunk):
    return ((cam.image_width + 7) // 8) * ((cam.image_height + 7) // 8) * 64 * -(-spp // chunk)


def render(gpu, cam, s):
    """(frame, (samples, segments), counters)."""
    img = gpu.render(cam, s)
    c = gpu.counters()
    assert c.engine == 1 and c.samples == cam.image_width * cam.image_height * s.samples
    return img, (int(c.samples), int(c.segments)), c


def chunked_oracle(osc, cam, spp, chunk):
    total = None
    for c in range(-(-spp // chunk)):
        n = min(chunk, spp - c * chunk)
        part, _ = osc.render(cam, O.params(spp, 50, SEED, sample_begin=c * chunk, sample_count=n), threads=16)
        total = part if total is None else total + part
    return total


def default_frame(gpu, scene, cache, width, height, spp, chunk):
    """The default distribution's frame of the case (checked against the chunked oracle frame when first made)."""
    key = (width, height, spp, chunk)
    if key not in cache:
        sc, osc = scene
        cam = frame_camera(width, height)
        gpu.upload(sc)
        img, cnt, _ = render(gpu, cam, settings(spp, chunk))
        check_parity(img, chunked_oracle(osc, cam, spp, chunk), spp)
        img.setflags(write=False)
        cache[key] = (cam, img, cnt)
    return cache[key]


def same_as_default(gpu, scene, cache, monkeypatch, size, spp, chunk, env, **kw):
    cam, want, want_cnt = default_frame(gpu, scene, cache, *size, spp, chunk)
    gpu.upload(scene[0])
    with switches(monkeypatch, **env):
        img, cnt, c = render(gpu, cam, settings(spp, chunk, **kw))
    assert np.array_equal(img, want), f"{int(np.sum(np.any(img != want, axis=-1)))} pixels differ under {env}"
    assert cnt == want_cnt
    return c


# ---- the shared queue: every window size, with a partial last window ----------------------------------------------
@pytest.mark.parametrize("window", [64, 256, 1024])
@pytest.mark.parametrize("size", [(40, 24), (37, 21)], ids=["40x24", "37x21"])
def test_shared_queue_window_sweep(gpu, scene, cache, monkeypatch, size, window):
    """One-sample units (the plan's shared queue).  5 x 3 tiles (37 x 21: a partial tile column and row) at 3 spp are
    45 x 64 units: no multiple of 256 or 1024, so the last window is partial."""
    spp, chunk = 3, 1
    units = n_units(frame_camera(*size), spp, chunk)
    assert units == 45 * 64 and units % 256 != 0 and units % 1024 != 0
    same_as_default(gpu, scene, cache, monkeypatch, size, spp, chunk, dict(WINDOW=window))


def test_segments_forced_on_short_units(gpu, scene, cache, monkeypatch):
    """One-sample units from per-block segments (the plan gives them the shared queue)."""
    same_as_default(gpu, scene, cache, monkeypatch, (40, 24), 3, 1, dict(SEGMENTS=1))


@pytest.mark.parametrize("window", [None, 256])
def test_queue_forced_on_long_units(gpu, scene, cache, monkeypatch, window):
    """Four-sample units from the shared queue (the plan gives them segments), with the last chunk short."""
    env = dict(SEGMENTS=0) if window is None else dict(SEGMENTS=0, WINDOW=window)
    same_as_default(gpu, scene, cache, monkeypatch, (40, 24), 10, 4, env)


# ---- segments longer than one window -------------------------------------------------------------------------------
BIG = (256, 136)  # 32 x 17 tiles
BIG_SPP, BIG_CHUNK = 16, 4


def big_units():
    import torch
    units = n_units(frame_camera(*BIG), BIG_SPP, BIG_CHUNK)
    # one segment per megakernel block, at most 4 blocks per CU: every segment holds more than one 64-unit window
    blocks = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    assert units == 139264 and units > 64 * blocks
    return units


@pytest.mark.parametrize("env", [dict(SEGMENTS=0), dict(SEGMENTS=0, WINDOW=256), dict(SEGMENTS=1)],
                         ids=["queue-64", "queue-256", "segments"])
def test_segments_of_several_windows(gpu, scene, cache, monkeypatch, env):
    """256 x 136 @ 16 spp in four-sample units: 139 264 units.  The default distribution (segments of several
    windows) against the chunked oracle frame over the whole frame (default_frame), and the queue against it."""
    big_units()
    c = same_as_default(gpu, scene, cache, monkeypatch, BIG, BIG_SPP, BIG_CHUNK, env)
    assert c.passes == 1 and c.n_chunks == 4


@pytest.mark.parametrize("env", [dict(), dict(SEGMENTS=0, WINDOW=256)], ids=["segments", "queue-256"])
def test_sample_passes_with_each_distribution(gpu, scene, cache, monkeypatch, env):
    """The same frame under a 1 MiB scratch bound (a chunk of it holds 835 584 bytes of partial sums): one pass per
    chunk, each its own launch with its own queue or segments."""
    big_units()
    c = same_as_default(gpu, scene, cache, monkeypatch, BIG, BIG_SPP, BIG_CHUNK, env, scratch_mb=1)
    assert c.passes > 1


# ---- tile shares ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [dict(WINDOW=256), dict(SEGMENTS=1)], ids=["queue-256", "segments"])
def test_tile_shares_with_each_distribution(gpu, scene, cache, monkeypatch, env):
    """tile_world = 3, every rank's packed tiles gathered and unpacked (as test_tiles_gather_unpack_equals_full_frame):
    the one-rank frame of the same chunk.  52 x 29: partial tiles on both axes, 28 tiles (ranks of 10, 9, 9)."""
    import torch
    spp, chunk, world = 3, 1, 3
    cam, want, _ = default_frame(gpu, scene, cache, 52, 29, spp, chunk)
    gpu.upload(scene[0])
    n_total, max_tiles = rt.tile_layout(cam, world)
    assert n_total == 28 and max_tiles == 10
    gathered = torch.zeros((world, max_tiles, 64, 3), dtype=torch.float64, device="cuda")
    samples = 0
    with switches(monkeypatch, **env):
        for r in range(world):
            gpu.render_tiles_device(cam, settings(spp, chunk, tile_rank=r, tile_world=world), gathered[r].data_ptr())
            gpu.synchronize()
            samples += int(gpu.counters().samples)
    accum = torch.zeros((cam.image_height, cam.image_width, 3), dtype=torch.float64, device="cuda")
    gpu.unpack_tiles_device(cam, world, gathered.data_ptr(), accum.data_ptr())
    gpu.synchronize()
    assert np.array_equal(accum.cpu().numpy(), want)
    assert samples == cam.image_width * cam.image_height * spp


# ---- tile lists ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def adaptive_shared(gpu, scene):
    """tests/test_gpu_adaptive.py's shared frames (its `shared` fixture) and the default distribution's mixed run."""
    cam = adaptive_camera()
    gpu.upload(scene[0])
    ref = {n: gpu.render(cam, rt.RenderSettings(**ADAPTIVE_BASE, sample_count=n)) for n in range(MIN, MAX + 1, STEP)}
    at_min = gpu.render_adaptive(cam, rt.RenderSettings(**ADAPTIVE_BASE), adaptive(float("inf")))
    sh = dict(cam=cam, ref=ref, at_min=at_min)
    thr = float(np.median(at_min[3]))
    check_adaptive(gpu, sh, thr)  # (the default run is the uniform frames' samples, tile by tile)
    sh["thr"] = thr
    sh["mixed"] = gpu.render_adaptive(cam, rt.RenderSettings(**ADAPTIVE_BASE), adaptive(thr))
    return sh


@pytest.mark.parametrize("env", [dict(WINDOW=256), dict(SEGMENTS=0), dict(SEGMENTS=0, WINDOW=256)],
                         ids=["window-256", "queue-64", "queue-256"])
def test_tile_lists_with_each_distribution(gpu, scene, adaptive_shared, monkeypatch, env):
    """One adaptive run at the median tile error (test_mixed_thresholds: half the tiles go on, so every later step
    renders a list): sums, counts, moments and tile errors equal the default distribution's.  The batches are
    four-sample units, so the plan serves them from segments and SHIRLEY_WINDOW alone changes nothing; with
    SHIRLEY_SEGMENTS=0 they come from the queue, in 64- and in 256-unit windows."""
    sh = adaptive_shared
    gpu.upload(scene[0])
    with switches(monkeypatch, **env):
        got = gpu.render_adaptive(sh["cam"], rt.RenderSettings(**ADAPTIVE_BASE), adaptive(sh["thr"]))
    want = sh["mixed"]
    assert len(np.unique(want[1])) > 1
    for name, a, b in zip(("accum", "counts", "moments", "tile_error"), got[:4], want[:4]):
        assert np.array_equal(a, b), f"{name} differs under {env}"
    for f in ("samples", "segments", "steps", "tiles", "tiles_converged"):
        assert getattr(got[4], f) == getattr(want[4], f), f
