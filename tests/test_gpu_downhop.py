"""The down pass of a scene with a ground stack (trace.hip step 1', HOP = 3; rt_device.h ground_hop_t<true>;
ScenePlacement.hop_down): a lane whose traversal hit is a dielectric primitive of the stack is
shaded before the sampler, hops down through the coat and takes the rect under it as this iteration's hit; a lane
the stack cannot answer waits for the next iteration's traversal.  Every lane still runs the same pure functions of
(seed, pixel, sample, draw index, ray) in the same order, so frames, per-unit partial sums (the frame's sample
ranges, one unit each) and the samples / segments counters must be bit-identical between four uploads: the default
(the down pass where the stack has a non-dielectric member below its coat), SHIRLEY_HOP=up (the ground-stack pass
alone), SHIRLEY_HOP=root (the first-node visit) and SHIRLEY_NO_HOP=1 (no pass).

random_scene's frames are 64x48 @ 8 spp in units of 3, 3 and 2 samples, from the two tests/hop_scenes.py camera
positions (straight down and from 7 degrees of elevation) on a patch of open coat, so whole waves meet the pass's
lane thresholds (tests/test_down_hop.py test_random_scene_frames_hold_down_candidates, by the oracle alone)."""
import numpy as np
import pytest

import hop_scenes as HS
import raytracer as rt
from test_down_hop import FRAME_H as H, FRAME_W as W, random_cameras
from test_gpu_hop import camera
from test_gpu_hop_scenes import oracle_frame, exact_floor
from test_gpu_parity import check_parity

pytestmark = pytest.mark.gpu
SEED = HS.SEED
ENV = {"down": {}, "up": {"SHIRLEY_HOP": "up"}, "root": {"SHIRLEY_HOP": "root"}, "off": {"SHIRLEY_NO_HOP": "1"}}
KIND = {"down": (1, 2), "up": (1, 2), "root": (1, 1), "off": (0, 0)}  # rt_scene_stats (hop_pass, hop_kind)
OTHERS = ("up", "root", "off")
SPP, CHUNK = 8, 3


def upload(gpu, monkeypatch, scene, mode):
    for k in ("SHIRLEY_NO_HOP", "SHIRLEY_HOP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ENV[mode].items():
        monkeypatch.setenv(k, v)
    gpu.upload(scene)
    for k in ("SHIRLEY_NO_HOP", "SHIRLEY_HOP"):
        monkeypatch.delenv(k, raising=False)
    st = gpu.stats()
    return st.hop_pass, st.hop_kind


def render_all(gpu, monkeypatch, scene, jobs, kind2=True):
    """{mode: [(frame, samples, segments) per (camera, settings) job]} of the four uploads."""
    res = {}
    for mode in ENV:
        want = KIND[mode] if kind2 or mode == "off" else (1, 1)
        assert upload(gpu, monkeypatch, scene, mode) == want, mode
        res[mode] = []
        for cam, s in jobs:
            img = gpu.render(cam, s)
            cnt = gpu.counters()
            res[mode].append((img, int(cnt.samples), int(cnt.segments)))
    return res


def assert_equal(res, labels):
    for k, label in enumerate(labels):
        a, a_samples, a_segments = res["down"][k]
        for other in OTHERS:
            b, b_samples, b_segments = res[other][k]
            assert np.array_equal(a, b), (label, other)
            assert (a_samples, a_segments) == (b_samples, b_segments), (label, other)


@pytest.fixture(scope="module")
def random_scene():
    return rt.scenes.random_scene(SEED).finalize(SEED)


def test_random_scene_frames_units_and_counters(gpu, monkeypatch, random_scene):
    """The whole frame (units of 3, 3 and 2 samples summed in order) and each unit's own partial sums — the sample
    ranges [0, 3), [3, 6), [6, 8) rendered alone — at depth 50 and at depths 1 .. 6, where a path dies at every
    position of the chain: on the coat's top, inside the coat, on the rect and on the way up."""
    cams = random_cameras()
    jobs, labels = [], []
    for c, cam in cams.items():
        for depth in (50, 1, 2, 3, 4, 5, 6):
            ranges = [(0, 0)] + ([(0, 3), (3, 3), (6, 2)] if depth in (50, 4) else [])
            for begin, count in ranges:
                jobs.append((cam, rt.RenderSettings(samples=SPP, max_reflect=depth, seed=SEED, sample_chunk=CHUNK,
                                                    sample_begin=begin, sample_count=count)))
                labels.append((c, depth, begin, count))
    res = render_all(gpu, monkeypatch, random_scene, jobs)
    gpu.upload(random_scene)
    assert_equal(res, labels)
    for k, (c, depth, begin, count) in enumerate(labels):
        assert res["down"][k][1] == W * H * (count or SPP), labels[k]
    # the units' partial sums, added in order, are the frame
    for c in cams:
        for depth in (50, 4):
            k = labels.index((c, depth, 0, 0))
            total = res["down"][k + 1][0] + res["down"][k + 2][0] + res["down"][k + 3][0]
            assert np.array_equal(total, res["down"][k][0]), (c, depth)


@pytest.mark.parametrize("name", HS.KIND2)
def test_modes_agree_on_a_ground_stack(gpu, monkeypatch, name):
    """Every ground-stack scene of tests/hop_scenes.py — tied, guarded, raised-rect and two-box stacks among them,
    and so the lanes the pass leaves waiting — both cameras, at depth 50 and at depths 1 .. 6 in units of one sample
    and of four; the default upload also meets the oracle's parity rule (tests/test_gpu_hop_scenes.py's)."""
    cams = HS.cameras(name)
    what = [(c, depth, chunk) for c in cams for depth, chunk in
            ((50, 4), (1, 1), (2, 4), (3, 1), (4, 4), (5, 1), (6, 4))]
    jobs = [(cams[c], rt.RenderSettings(samples=4, max_reflect=depth, seed=SEED, sample_chunk=chunk))
            for c, depth, chunk in what]
    res = render_all(gpu, monkeypatch, HS.scene(name), jobs)
    assert_equal(res, what)
    for k, (c, depth, chunk) in enumerate(what):
        assert res["down"][k][1] == 32 * 32 * 4
        if (depth, chunk) == (50, 4):
            check_parity(res["down"][k][0], oracle_frame(name, c), 4, frac_exact=exact_floor(f"{name}:reference:{c}"))


@pytest.mark.parametrize("name", HS.KIND1)
def test_no_ground_stack_no_down_pass(gpu, monkeypatch, name):
    """A scene without a ground stack runs the first-node pass under the default upload and under SHIRLEY_HOP=up."""
    cams = HS.cameras(name)
    jobs = [(cams[c], rt.RenderSettings(samples=4, max_reflect=50, seed=SEED, sample_chunk=4)) for c in cams]
    res = render_all(gpu, monkeypatch, HS.scene(name), jobs, kind2=False)
    assert_equal(res, list(cams))


def test_list_instance(gpu, monkeypatch, random_scene):
    """rt_render_adaptive with threshold 0 — the second step's launch names every tile in a list — on the down
    pass's LIST instance against the other three uploads."""
    cam = camera(48, 32)
    s = rt.RenderSettings(samples=16, seed=SEED, sample_chunk=4)
    a = rt.AdaptiveSettings(threshold=0.0, min_samples=8, step=8, noise_floor=0.01)
    res = {}
    for mode in ENV:
        assert upload(gpu, monkeypatch, random_scene, mode) == KIND[mode]
        res[mode] = gpu.render_adaptive(cam, s, a)
    gpu.upload(random_scene)
    for other in OTHERS:
        assert res["down"][4].steps == res[other][4].steps == 2
        for x, y in zip(res["down"][:4], res[other][:4]):
            assert np.array_equal(x, y), other
        assert (res["down"][4].samples, res["down"][4].segments) == (res[other][4].samples, res[other][4].segments)
