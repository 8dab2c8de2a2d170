"""The serve body written out for a y face (rt_device.h serve_y; trace.hip HOP = 4, RT_SERVE_Y): the
down pass and step 5' of a plane stack's instance shade a dielectric hit on face 4 or 5 of a RectBox with the axis
normal written out, and every other lane — a side face, a zero or tiny component — by the general body.  Same bits
either way, so frames, per-unit partial sums and the samples / segments counters must be bit-identical between the
five uploads of tests/test_gpu_planehop.py: the default (instance 4, the only one with serve_y), SHIRLEY_HOP=general
(3: the general serve body in both passes), SHIRLEY_HOP=up (2), SHIRLEY_HOP=root (1) and SHIRLEY_NO_HOP=1 (none: every
dielectric hit shaded by shade_factor).

Frames: random_scene at 200x112 @ 8 spp; every plane stack of tests/hop_scenes.py — two_coats among them, glass boxes
of 1.3 and 1.5 with a rect between, where a served hit from inside a box can reflect totally — from that module's two
on-the-coat cameras at 64x64 @ 4 spp (64 waves of coat pixels, so whole waves run both passes)."""
import numpy as np
import pytest

import hop_scenes as HS
import raytracer as rt
from test_gpu_hop import camera
from test_gpu_hop_scenes import scene
from test_gpu_planehop import assert_equal, render_all
from test_plane_hop import PLANE

pytestmark = pytest.mark.gpu
SEED = HS.SEED
W = 64


def cameras(name):
    """tests/hop_scenes.py cameras(name) — straight down from 1.25 above ball 0's contact point, and from 7 degrees of
    elevation at 0.875 from it — on a 64x64 frame."""
    y = HS.CAMERA_Y.get(name, 0.0)
    x, z = HS.CAMERA_XZ.get((name, "down"), HS.ball_xz(0))
    down = rt.CameraBuilder(width=W, aspect_ratio=(W, W), vfov=30.0, focal_length=1.0, aperture=0.001).build(
        rt.CameraPosition((x, y + 1.25, z), (x, y, z), (0.0, 0.0, -1.0), focus_length=1.25))
    x, z = HS.CAMERA_XZ.get((name, "low"), HS.ball_xz(0))
    e = np.radians(7.0)
    low = rt.CameraBuilder(width=W, aspect_ratio=(W, W), vfov=8.0, focal_length=1.0, aperture=0.001).build(
        rt.CameraPosition((x + 0.875 * np.cos(e), y + 0.875 * np.sin(e), z), (x, y, z), (0.0, 1.0, 0.0), focus_length=0.875))
    assert (down.image_width, down.image_height, low.image_width, low.image_height) == (W, W, W, W)
    return {"down": down, "low": low}


@pytest.mark.parametrize("name", PLANE)
def test_modes_agree_on_a_plane_stack(gpu, monkeypatch, name):
    """Both cameras at depth 50 in one unit of four samples and in units of one, the four samples as units of their own
    (the per-unit sums), and depths 2 and 3, where a path dies inside the coat and on the rect — the death decision
    that follows a served hit."""
    cams = cameras(name)
    what = [(c, depth, chunk, 0, 0) for c in cams for depth, chunk in ((50, 4), (50, 1), (2, 4), (3, 1))]
    what += [(c, 50, 1, k, 1) for c in cams for k in range(4)]
    jobs = [(cams[c], rt.RenderSettings(samples=4, max_reflect=depth, seed=SEED, sample_chunk=chunk, sample_begin=begin,
                                        sample_count=count)) for c, depth, chunk, begin, count in what]
    res = render_all(gpu, monkeypatch, scene(name), jobs)
    assert_equal(res, what)
    for k, (c, depth, chunk, begin, count) in enumerate(what):
        assert res["planes"][k][1] == W * W * (count or 4)
    for c in cams:  # the units' sums, added in order, are the frame rendered in units of one sample
        k, u = what.index((c, 50, 1, 0, 0)), what.index((c, 50, 1, 0, 1))
        total = res["planes"][u][0] + res["planes"][u + 1][0] + res["planes"][u + 2][0] + res["planes"][u + 3][0]
        assert np.array_equal(total, res["planes"][k][0]), c
    # (render_all checks rt_scene_hop_instance per upload: the default one does run the instance with serve_y)


def test_random_scene_frame_units_and_counters(gpu, monkeypatch):
    """random_scene at 200x112 @ 8 spp, depth 50: the frame (units of 3, 3 and 2 samples summed in order), each unit's
    own partial sums, and the counters."""
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
