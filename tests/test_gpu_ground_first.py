"""The traversal's closed-form answer about a plane stack on the device (trace.hip HOP = 4 with RT_GROUND_FIRST;
rt_device.h plane_first, traverse4 GF): before its first visit a ray of the two HOP = 4 instances
settles what the stack's rects and RectBoxes can return — none, or the first plane ahead — starts its loop from that
answer and skips those leaves; a ray outside the premises declines and runs the leaf tests as before.  The closest
hit is the same pure function of the ray either way, so frames, per-unit partial sums and the samples / segments
counters must be bit-identical between five uploads: the default (instance 4, the only one with the new code),
SHIRLEY_HOP=general (3), SHIRLEY_HOP=up (2), SHIRLEY_HOP=root (1) and SHIRLEY_NO_HOP=1 (0) — the device-side
references.

Frames: random_scene at 200x112 @ 8 spp; every plane stack of tests/hop_scenes.py and tests/ground_first_scenes.py's
big_ball (a sphere that is a leaf child of the first node visited, beside the stack's leaves) at 64x64 @ 8 spp from
six cameras — the two on-the-coat ones, straight down from just below and just above the origin-height bound H,
grazing along the coat beyond the slope bound (whole waves decline), and pulled back until the frame shows the
stack's edge (hit points outside the core, rays over the edge)."""
import numpy as np
import pytest

import ground_first_scenes as GS
import raytracer as rt
from test_gpu_hop import camera
from test_gpu_planehop import assert_equal, render_all
from test_plane_hop import PLANE

pytestmark = pytest.mark.gpu
SEED = GS.SEED


@pytest.mark.parametrize("name", PLANE + GS.NAMES)
def test_modes_agree_on_a_plane_stack(gpu, monkeypatch, name):
    """Every camera at depth 50, 8 spp in units of 3, 3 and 2 samples, and at depth 2 (paths that die on their second
    segment: the answer of the first traversal alone decides the frame); the first unit rendered alone too."""
    cams = GS.cameras(name)
    what = [(c, depth, begin, count) for c in GS.CAMERAS for depth, begin, count in ((50, 0, 0), (2, 0, 0), (50, 0, 3))]
    jobs = [(cams[c], rt.RenderSettings(samples=8, max_reflect=depth, seed=SEED, sample_chunk=3, sample_begin=begin,
                                        sample_count=count)) for c, depth, begin, count in what]
    res = render_all(gpu, monkeypatch, GS.scene(name), jobs)
    assert_equal(res, what)
    for k, (c, depth, begin, count) in enumerate(what):
        assert res["planes"][k][1] == 64 * 64 * (count or 8)
    # the frames are not trivially equal: each camera sees something, and the cameras differ
    frames = [res["planes"][what.index((c, 50, 0, 0))][0] for c in GS.CAMERAS]
    assert all(float(f.max()) > 0.0 for f in frames)
    assert not np.array_equal(frames[GS.CAMERAS.index("high")], frames[GS.CAMERAS.index("back")])


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
