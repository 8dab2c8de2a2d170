"""The megakernel's hop pass (trace.hip step 5): a lane that goes on from a rect or RectBox
hit tries its next segment at the end of the same iteration, and finishes it there when the tree's first
node decides the closest hit and that hit is a dielectric.  Each lane runs the same pure functions of (seed,
pixel, sample, draw index, ray) in the same order with the pass and without it, so frames and the samples /
segments counters must be bit-identical between the default upload (rt_scene_stats.hop_pass = 1 for a
reference scene held in LDS with a dielectric RectBox) and an upload under SHIRLEY_NO_HOP=1."""
import json

import numpy as np
import pytest

import oracle_lib as O
import raytracer as rt
from test_gpu_parity import PARITY_OUTLIERS, check_parity

pytestmark = pytest.mark.gpu
SEED = 0x5EED
SPP = 4


def camera(width, height):
    # default_camera's position and lens (scenes.rs:214-231) on a width x height frame
    cam = rt.CameraBuilder(width=width, aspect_ratio=(width, height), vfov=20.0, focal_length=1.0,
                           aperture=0.001).build(
        rt.CameraPosition((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), focus_length=10.0))
    assert (cam.image_width, cam.image_height) == (width, height)
    return cam


def ground_camera(width, height):
    """Looking down at the ground between the spheres: every pixel's path starts on the coat, so whole waves are
    hop candidates (measured with the instrumented build, profiles/hop/phase_k40_tests.txt: the pass runs in
    most iterations of this frame, against 84 of 5966 on the default camera's 48x27 frame)."""
    cam = rt.CameraBuilder(width=width, aspect_ratio=(width, height), vfov=30.0, focal_length=1.0,
                           aperture=0.001).build(
        rt.CameraPosition((3.0, 8.0, 2.0), (2.0, 0.0, 2.0), (0.0, 1.0, 0.0), focus_length=8.0))
    assert (cam.image_width, cam.image_height) == (width, height)
    return cam


def upload(gpu, monkeypatch, scene, hop, **kw):
    """Upload with the pass on (the default) or off (SHIRLEY_NO_HOP, read at upload); returns hop_pass."""
    if hop:
        monkeypatch.delenv("SHIRLEY_NO_HOP", raising=False)
    else:
        monkeypatch.setenv("SHIRLEY_NO_HOP", "1")
    gpu.upload(scene, **kw)
    monkeypatch.delenv("SHIRLEY_NO_HOP", raising=False)
    return gpu.stats().hop_pass


@pytest.fixture(scope="module")
def scene():
    return rt.scenes.random_scene(SEED).finalize(SEED)


@pytest.fixture(scope="module")
def oracle_frame(scene):
    """The oracle's 52x28 @ 4 spp frame at depth 50 (computed once)."""
    ora, _ = O.OracleScene(scene).render(camera(52, 28), O.params(SPP, 50, SEED), threads=16)
    ora.setflags(write=False)
    return ora


def test_on_off_equality(gpu, monkeypatch, scene, oracle_frame):
    # 52x28: 7 x 4 tiles, the last column and the last row partial (lanes without units); depths at which
    # paths die inside a hop; units of one sample and of all four
    # the same on the ground camera, where the pass serves most ground segments (the default camera's small
    # frame runs it in about one iteration of seventy)
    cams = {"default": camera(52, 28), "ground": ground_camera(52, 28)}
    settings = [(c, rt.RenderSettings(samples=SPP, max_reflect=depth, seed=SEED, sample_chunk=chunk))
                for c in cams for depth in (1, 2, 3, 50) for chunk in (1, 4)]
    res = {}
    for hop in (True, False):
        assert upload(gpu, monkeypatch, scene, hop) == (1 if hop else 0)
        res[hop] = []
        for c, s in settings:
            img = gpu.render(cams[c], s)
            cnt = gpu.counters()
            res[hop].append((img, int(cnt.samples), int(cnt.segments)))
    gpu.upload(scene)
    for (c, s), (a, a_samples, a_segments), (b, b_samples, b_segments) in zip(settings, res[True], res[False]):
        what = (c, s.max_reflect, s.sample_chunk)
        assert np.array_equal(a, b), what
        assert a_samples == b_samples == 52 * 28 * SPP, what
        assert a_segments == b_segments, what
        if what == ("default", 50, 4):  # (sample_chunk = spp: the oracle's in-order sums)
            check_parity(a, oracle_frame, SPP)
            check_parity(b, oracle_frame, SPP)


def test_ties_fall_back(gpu, monkeypatch):
    """random_scene with every object twice (tests/test_gpu_ties.py): every hit is an exact tie, so a hop's
    first-node visit ends with the tie mark set and the lane falls back to the ordinary traversal.  (Measured:
    with twice the objects the scene no longer fits the scene-in-LDS instance, so today hop_pass is 0 for both
    uploads and the two frames come from the same kernel; the comparison holds whichever way the flag falls.)"""
    src = json.loads(rt.scenes.random_scene(SEED).to_json())
    red = {"Lambertian": {"albedo": {"Solid": {"vec": [0.9, 0.1, 0.05]}}}}
    objs = []
    for o in src["objects"]:
        objs.append(o)
        objs.append({**o, "material": red})
    src["objects"] = objs
    tied = rt.SceneBuilder.from_json(json.dumps(src)).finalize(SEED)
    cam = camera(32, 32)
    s = rt.RenderSettings(samples=SPP, max_reflect=50, seed=SEED, sample_chunk=SPP)
    res = {}
    for hop in (True, False):
        flag = upload(gpu, monkeypatch, tied, hop)
        assert flag == 0 or hop
        img = gpu.render(cam, s)
        cnt = gpu.counters()
        res[hop] = (img, int(cnt.samples), int(cnt.segments), flag)
    print("tied scene hop_pass (default upload):", res[True][3])
    assert np.array_equal(res[True][0], res[False][0])
    assert res[True][1:3] == res[False][1:3]


def tied_scene_in_lds(coat_copy):
    """The construction above on every third sphere, the rect and the coat: every hit still an exact tie, and
    the scene small enough for the scene-in-LDS instance, so the pass is on (random_scene itself fills 159 of
    the block's 160 KiB: two more objects already push it out).  coat_copy: "lambertian" — the coat's copy is
    red like every other copy — or "dielectric": the copy keeps the coat's material, so whichever of the pair
    wins, the hit is one the pass would serve, and only the tie mark stands between the visit and a hop."""
    src = json.loads(rt.scenes.random_scene(SEED).to_json())
    red = {"Lambertian": {"albedo": {"Solid": {"vec": [0.9, 0.1, 0.05]}}}}
    objs, n_spheres = [], 0
    for o in src["objects"]:
        if "Sphere" in o["geometry"]:
            n_spheres += 1
            if n_spheres % 3:
                continue
        objs.append(o)
        objs.append(o if coat_copy == "dielectric" and "RectBox" in o["geometry"] else {**o, "material": red})
    src["objects"] = objs
    return rt.SceneBuilder.from_json(json.dumps(src)).finalize(SEED)


@pytest.mark.parametrize("coat_copy", ["lambertian", "dielectric"])
@pytest.mark.parametrize("bvh", ["reference", "sah"])
def test_ties_fall_back_with_the_pass_on(gpu, monkeypatch, bvh, coat_copy):
    """Every hit a tie with hop_pass = 1: a hop whose first-node visit ends with the tie mark set (a tied leaf
    whose box fails at the closest t by rounding, mark_tie) must fall back to the ordinary traversal and its
    resolve pass (traverse4_root's `!(best & kTieBit)`).
    On both cameras: on and off bit-identical, and the frame follows the oracle's choice of every tie.
    The instrumented build on these frames (profiles/hop/phase_k40_tests.txt): the pass runs 33 / 60 times with
    the Lambertian copy and 134 / 308 times with the dielectric one (default / ground camera, 1740 to 18 750
    candidate visits) and serves nothing: every coat hit's visit ends marked (the twin's box fails hit2 at the
    tie), so each of those lanes goes through the tie guard to the ordinary traversal and its resolve pass.
    Oracle gate: the Lambertian copy, the scene set first, passes the whole parity rule.  The dielectric copy
    measured 0.97656 bit-identical channels at a largest difference of 8.9e-16 on one camera — last-bit libm
    differences on a frame that is mostly coat, below the rule's 0.99, with and without the pass alike — so
    there the test holds the half of the rule that a wrong tie winner breaks: a flipped path moves a sample by
    its radiance, far beyond 1e-10 * spp, on at most 0.1 % of pixels."""
    tied = tied_scene_in_lds(coat_copy)
    s = rt.RenderSettings(samples=SPP, max_reflect=50, seed=SEED, sample_chunk=SPP)
    cams = {"default": camera(32, 32), "ground": ground_camera(32, 32)}
    res = {}
    for hop in (True, False):
        assert upload(gpu, monkeypatch, tied, hop, bvh=bvh) == (1 if hop else 0)
        for c, cam in cams.items():
            img = gpu.render(cam, s)
            cnt = gpu.counters()
            res[hop, c] = (img, int(cnt.samples), int(cnt.segments))
    for c, cam in cams.items():
        assert np.array_equal(res[True, c][0], res[False, c][0]), c
        assert res[True, c][1:] == res[False, c][1:], c
        ora, _ = O.OracleScene(tied).render(cam, O.params(SPP, 50, SEED), threads=16)
        img = res[True, c][0]
        print(f"{coat_copy} {bvh} {c}: bit-identical channels {np.mean(img == ora):.5f}, max |gpu - oracle| "
              f"{np.abs(img - ora).max():.3g}")
        if coat_copy == "lambertian":
            check_parity(img, ora, SPP)
        else:
            assert np.mean(np.any(np.abs(img - ora) > 1e-10 * SPP, axis=-1)) <= PARITY_OUTLIERS, c


def test_list_twin(gpu, monkeypatch, scene):
    # an adaptive run with threshold 0 — no tile converges, so the second step's launch names every tile in a
    # list (the LIST instance)
    cam = camera(48, 32)
    s = rt.RenderSettings(samples=16, seed=SEED, sample_chunk=4)
    a = rt.AdaptiveSettings(threshold=0.0, min_samples=8, step=8, noise_floor=0.01)
    res = {}
    for hop in (True, False):
        assert upload(gpu, monkeypatch, scene, hop) == (1 if hop else 0)
        res[hop] = gpu.render_adaptive(cam, s, a)
    gpu.upload(scene)
    assert res[True][4].steps == res[False][4].steps == 2
    for x, y in zip(res[True][:4], res[False][:4]):
        assert np.array_equal(x, y)
    assert (res[True][4].samples, res[True][4].segments) == (res[False][4].samples, res[False][4].segments)


@pytest.mark.parametrize("name", ["cornell", "earth"])
def test_flag_off_elsewhere(gpu, monkeypatch, name):
    monkeypatch.delenv("SHIRLEY_NO_HOP", raising=False)
    gpu.upload(rt.SceneBuilder.builtin(name, SEED).finalize(SEED))
    assert gpu.stats().hop_pass == 0
