"""The hop pass of a scene with a ground stack (trace.hip step 5', rt_device.h ground_hop): a
candidate's closest hit comes from the stack's own rects and RectBoxes, without a node visit, and is served where
the stack's conditions prove it the scene's closest hit; the pass runs twice per iteration.  Every lane still
runs the same pure functions of (seed, pixel, sample, draw index, ray) in the same order, so frames and the
samples / segments counters must be bit-identical between the three uploads: the default (rt_scene_stats.hop_kind
= 2 for random_scene), SHIRLEY_HOP=root (1: the first-node visit) and SHIRLEY_NO_HOP=1 (0)."""
import json

import numpy as np
import pytest

import oracle_lib as O
import raytracer as rt
from test_gpu_hop import camera, ground_camera, tied_scene_in_lds
from test_gpu_parity import PARITY_OUTLIERS, check_parity

pytestmark = pytest.mark.gpu
SEED = 0x5EED
SPP = 4
MODES = {"off": 0, "root": 1, "ground": 2}


def upload(gpu, monkeypatch, scene, mode, **kw):
    """Upload under the mode's environment (read at upload); returns rt_scene_stats (hop_pass, hop_kind)."""
    monkeypatch.delenv("SHIRLEY_NO_HOP", raising=False)
    monkeypatch.delenv("SHIRLEY_HOP", raising=False)
    if mode == "off":
        monkeypatch.setenv("SHIRLEY_NO_HOP", "1")
    elif mode == "root":
        monkeypatch.setenv("SHIRLEY_HOP", "root")
    gpu.upload(scene, **kw)
    monkeypatch.delenv("SHIRLEY_NO_HOP", raising=False)
    monkeypatch.delenv("SHIRLEY_HOP", raising=False)
    st = gpu.stats()
    return st.hop_pass, st.hop_kind


@pytest.fixture(scope="module")
def scene():
    return rt.scenes.random_scene(SEED).finalize(SEED)


def render_modes(gpu, monkeypatch, scene, jobs, modes=("ground", "root", "off"), **kw):
    """{mode: [(frame, samples, segments) per (camera, settings) job]}, each mode's kind checked at upload."""
    res = {}
    for mode in modes:
        assert upload(gpu, monkeypatch, scene, mode, **kw) == (1 if MODES[mode] else 0, MODES[mode]), mode
        res[mode] = []
        for cam, s in jobs:
            img = gpu.render(cam, s)
            cnt = gpu.counters()
            res[mode].append((img, int(cnt.samples), int(cnt.segments)))
    return res


def test_three_modes_equal(gpu, monkeypatch, scene):
    # 52x28: 7 x 4 tiles, the last column and row partial; depths at which a path dies inside the first or the
    # second run of the pass; units of one sample and of all four; the ground camera runs the pass in most
    # iterations
    cams = {"default": camera(52, 28), "ground": ground_camera(52, 28)}
    what = [(c, depth, chunk) for c in cams for depth in (1, 2, 3, 50) for chunk in (1, 4)]
    jobs = [(cams[c], rt.RenderSettings(samples=SPP, max_reflect=depth, seed=SEED, sample_chunk=chunk))
            for c, depth, chunk in what]
    res = render_modes(gpu, monkeypatch, scene, jobs)
    gpu.upload(scene)
    for k, w in enumerate(what):
        a, a_samples, a_segments = res["ground"][k]
        for other in ("root", "off"):
            b, b_samples, b_segments = res[other][k]
            assert np.array_equal(a, b), (w, other)
            assert a_samples == b_samples == 52 * 28 * SPP, (w, other)
            assert a_segments == b_segments, (w, other)
        if w == ("default", 50, 4):  # (sample_chunk = spp: the oracle's in-order sums)
            ora, _ = O.OracleScene(scene).render(cams["default"], O.params(SPP, 50, SEED), threads=16)
            check_parity(a, ora, SPP)


def guard_cameras(scene_json):
    """Two 32x32 cameras on the contact point of the first sphere of radius 0.15 .. 0.25 that has no neighbour
    within 0.6: straight down from 1.2 above it — the sphere's cap in the middle, the coat around it — and from
    7 degrees above the ground at 0.9, from where the coat inside the guard radius (1/32) under the sphere's
    overhang is in view (a ray at elevation e reaches the ground at distance rho from the contact point when
    tan e <= 2 rho / r), so guarded exits and served ones fall in the same waves."""
    spheres = [(o["geometry"]["Sphere"]["center"]["vec"], o["geometry"]["Sphere"]["radius"])
               for o in json.loads(scene_json)["objects"] if "Sphere" in o["geometry"]]
    for c, r in spheres:
        near = [1 for c2, r2 in spheres if c2 is not c and np.hypot(c2[0] - c[0], c2[2] - c[2]) < 0.6 + abs(r2)]
        if 0.15 <= r <= 0.25 and not near:
            break
    else:
        raise AssertionError("no isolated small sphere")
    at = (c[0], 0.0, c[2])
    down = rt.CameraBuilder(width=32, aspect_ratio=(32, 32), vfov=30.0, focal_length=1.0, aperture=0.001).build(
        rt.CameraPosition((c[0], 1.2, c[2]), at, (0.0, 0.0, -1.0), focus_length=1.2))
    e = np.radians(7.0)
    low = rt.CameraBuilder(width=32, aspect_ratio=(32, 32), vfov=8.0, focal_length=1.0, aperture=0.001).build(
        rt.CameraPosition((c[0] + 0.9 * np.cos(e), 0.9 * np.sin(e), c[2]), at, (0.0, 1.0, 0.0), focus_length=0.9))
    return {"down": down, "low": low}


def test_guard_camera(gpu, monkeypatch, scene):
    cams = guard_cameras(rt.scenes.random_scene(SEED).to_json())
    s = rt.RenderSettings(samples=SPP, max_reflect=50, seed=SEED, sample_chunk=SPP)
    res = render_modes(gpu, monkeypatch, scene, [(cam, s) for cam in cams.values()])
    gpu.upload(scene)
    for k, (name, cam) in enumerate(cams.items()):
        for other in ("root", "off"):
            assert np.array_equal(res["ground"][k][0], res[other][k][0]), (name, other)
            assert res["ground"][k][1:] == res[other][k][1:], (name, other)
        ora, _ = O.OracleScene(scene).render(cam, O.params(SPP, 50, SEED), threads=16)
        img = res["ground"][k][0]
        print(f"{name}: bit-identical channels {np.mean(img == ora):.5f}, max |gpu - oracle| {np.abs(img - ora).max():.3g}")
        check_parity(img, ora, SPP)


@pytest.mark.parametrize("coat_copy", ["lambertian", "dielectric"])
@pytest.mark.parametrize("bvh", ["reference", "sah"])
def test_tied_scenes(gpu, monkeypatch, bvh, coat_copy):
    """Both scenes of tests/test_gpu_hop.py tied_scene_in_lds (every hit an exact tie; a ground stack of four),
    both trees: the ground pass against no pass bit-identical, with test_ties_fall_back_with_the_pass_on's oracle
    gates — the whole parity rule for the Lambertian copy; for the dielectric one, whose frames measure 0.977
    bit-identical channels with and without any pass, the half a wrong tie winner breaks."""
    tied = tied_scene_in_lds(coat_copy)
    s = rt.RenderSettings(samples=SPP, max_reflect=50, seed=SEED, sample_chunk=SPP)
    cams = {"default": camera(32, 32), "ground": ground_camera(32, 32)}
    res = render_modes(gpu, monkeypatch, tied, [(cam, s) for cam in cams.values()], modes=("ground", "off"), bvh=bvh)
    for k, (c, cam) in enumerate(cams.items()):
        assert np.array_equal(res["ground"][k][0], res["off"][k][0]), c
        assert res["ground"][k][1:] == res["off"][k][1:], c
        ora, _ = O.OracleScene(tied).render(cam, O.params(SPP, 50, SEED), threads=16)
        img = res["ground"][k][0]
        print(f"{coat_copy} {bvh} {c}: bit-identical channels {np.mean(img == ora):.5f}, max |gpu - oracle| "
              f"{np.abs(img - ora).max():.3g}")
        if coat_copy == "lambertian":
            check_parity(img, ora, SPP)
        else:
            assert np.mean(np.any(np.abs(img - ora) > 1e-10 * SPP, axis=-1)) <= PARITY_OUTLIERS, c


def test_list_twin(gpu, monkeypatch, scene):
    # test_gpu_hop.py's adaptive run with threshold 0 (the second step's launch names every tile in a list) on
    # the ground-stack LIST instance, against no pass
    cam = camera(48, 32)
    s = rt.RenderSettings(samples=16, seed=SEED, sample_chunk=4)
    a = rt.AdaptiveSettings(threshold=0.0, min_samples=8, step=8, noise_floor=0.01)
    res = {}
    for mode in ("ground", "off"):
        assert upload(gpu, monkeypatch, scene, mode) == (1 if MODES[mode] else 0, MODES[mode])
        res[mode] = gpu.render_adaptive(cam, s, a)
    gpu.upload(scene)
    assert res["ground"][4].steps == res["off"][4].steps == 2
    for x, y in zip(res["ground"][:4], res["off"][:4]):
        assert np.array_equal(x, y)
    assert (res["ground"][4].samples, res["ground"][4].segments) == (res["off"][4].samples, res["off"][4].segments)
