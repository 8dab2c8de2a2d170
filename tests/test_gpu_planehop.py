"""The hop passes of a plane stack (trace.hip HOP = 4; rt_device.h plane_hop_t; ScenePlacement.hop_planes; DESIGN.md
§3.1): where a ground stack's y planes lie a gap apart inside a common xz core, the down pass and step 5' take the
stack's answer from the closed-form next plane instead of the general leaf machinery — the same answer, or none (the
lane then waits or traverses as before).  Every lane still runs the same pure functions of (seed, pixel, sample, draw
index, ray) in the same order, so frames, per-unit partial sums and the samples / segments counters must be
bit-identical between five uploads: the default (instance 4), SHIRLEY_HOP=general (3: the general passes),
SHIRLEY_HOP=up (2), SHIRLEY_HOP=root (1) and SHIRLEY_NO_HOP=1 (0).  rt_scene_hop_instance says which instance an
upload runs, so the comparison is not vacuous; rt_scene_stats.hop_kind is what it was.

Frames: every plane-stack scene of tests/hop_scenes.py from its two whole-wave-on-the-coat cameras, 32x32 @ 4 spp as
in tests/test_gpu_hop_scenes.py, and random_scene at 200x112 @ 8 spp, depth 50."""
import numpy as np
import pytest

import hop_scenes as HS
import raytracer as rt
from test_gpu_hop import camera
from test_gpu_hop_scenes import scene
from test_plane_hop import NOT_PLANE, PLANE

pytestmark = pytest.mark.gpu
SEED = HS.SEED
ENV = {"planes": {}, "general": {"SHIRLEY_HOP": "general"}, "up": {"SHIRLEY_HOP": "up"}, "root": {"SHIRLEY_HOP": "root"},
       "off": {"SHIRLEY_NO_HOP": "1"}}
# (rt_scene_stats hop_pass, hop_kind, rt_scene_hop_instance) of a plane stack's five uploads
KIND = {"planes": (1, 2, 4), "general": (1, 2, 3), "up": (1, 2, 2), "root": (1, 1, 1), "off": (0, 0, 0)}
OTHERS = ("general", "up", "root", "off")


def upload(gpu, monkeypatch, sc, mode):
    for k in ("SHIRLEY_NO_HOP", "SHIRLEY_HOP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ENV[mode].items():
        monkeypatch.setenv(k, v)
    gpu.upload(sc)
    for k in ("SHIRLEY_NO_HOP", "SHIRLEY_HOP"):
        monkeypatch.delenv(k, raising=False)
    st = gpu.stats()
    return st.hop_pass, st.hop_kind, gpu.hop_instance()


def render_all(gpu, monkeypatch, sc, jobs):
    """{mode: [(frame, samples, segments) per (camera, settings) job]} of the five uploads."""
    res = {}
    for mode in ENV:
        assert upload(gpu, monkeypatch, sc, mode) == KIND[mode], mode
        res[mode] = []
        for cam, s in jobs:
            img = gpu.render(cam, s)
            cnt = gpu.counters()
            res[mode].append((img, int(cnt.samples), int(cnt.segments)))
    return res


def assert_equal(res, labels):
    for k, label in enumerate(labels):
        a, a_samples, a_segments = res["planes"][k]
        for other in OTHERS:
            b, b_samples, b_segments = res[other][k]
            assert np.array_equal(a, b), (label, other)
            assert (a_samples, a_segments) == (b_samples, b_segments), (label, other)


@pytest.mark.parametrize("name", PLANE)
def test_modes_agree_on_a_plane_stack(gpu, monkeypatch, name):
    """Both cameras at depth 50 in one unit of four samples, the four samples as units of their own (sample ranges
    [k, k + 1) rendered alone: the per-unit sums), and depths 1 .. 4, where a path dies on the coat's top, inside
    the coat, on the rect and on the way up."""
    cams = HS.cameras(name)
    what = [(c, depth, chunk, 0, 0) for c in cams for depth, chunk in ((50, 4), (50, 1), (1, 1), (2, 4), (3, 1), (4, 4))]
    what += [(c, 50, 1, k, 1) for c in cams for k in range(4)]
    jobs = [(cams[c], rt.RenderSettings(samples=4, max_reflect=depth, seed=SEED, sample_chunk=chunk, sample_begin=begin,
                                        sample_count=count)) for c, depth, chunk, begin, count in what]
    res = render_all(gpu, monkeypatch, scene(name), jobs)
    assert_equal(res, what)
    for k, (c, depth, chunk, begin, count) in enumerate(what):
        assert res["planes"][k][1] == 32 * 32 * (count or 4)
    for c in cams:  # the units' sums, added in order, are the frame rendered in units of one sample
        k, u = what.index((c, 50, 1, 0, 0)), what.index((c, 50, 1, 0, 1))
        total = res["planes"][u][0] + res["planes"][u + 1][0] + res["planes"][u + 2][0] + res["planes"][u + 3][0]
        assert np.array_equal(total, res["planes"][k][0]), c


def test_random_scene_frame_units_and_counters(gpu, monkeypatch):
    """random_scene at 200x112 @ 8 spp, depth 50: the frame (units of 3, 3 and 2 samples summed in order) and each
    unit's own partial sums."""
    sc = rt.scenes.random_scene(SEED).finalize(SEED)
    cam = camera(200, 112)
    what = [(0, 0), (0, 3), (3, 3), (6, 2)]
    jobs = [(cam, rt.RenderSettings(samples=8, max_reflect=50, seed=SEED, sample_chunk=3, sample_begin=begin,
                                    sample_count=count)) for begin, count in what]
    res = render_all(gpu, monkeypatch, sc, jobs)
    gpu.upload(sc)  # (the session's shared device goes on with a default upload, not SHIRLEY_NO_HOP's)
    assert_equal(res, what)
    for k, (begin, count) in enumerate(what):
        assert res["planes"][k][1] == 200 * 112 * (count or 8)
    total = res["planes"][1][0] + res["planes"][2][0] + res["planes"][3][0]
    assert np.array_equal(total, res["planes"][0][0])


@pytest.mark.parametrize("name", NOT_PLANE + HS.KIND1)
def test_other_stacks_keep_their_instance(gpu, monkeypatch, name):
    """A ground stack that misses a premise of the plane stack — a core that does not contain the guard rectangle,
    two planes closer than the gap — keeps the general passes (instance 3, kind 2), under the default upload and
    under SHIRLEY_HOP=general alike; a scene without a ground stack keeps the first-node visit (1, kind 1)."""
    want = (1, 1, 1) if name in HS.KIND1 else (1, 2, 3)
    for mode in ("planes", "general"):
        assert upload(gpu, monkeypatch, scene(name), mode) == want, mode
