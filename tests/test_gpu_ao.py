"""rt_render_ao (occlusion.hip; include/shirley_rt.h ABI 11) against the CPU oracle's restatement of its
definition (tests/ao_ref.py).  The sums are integers and every decision behind them is an exact f64 test, so
every comparison is exact equality over the whole frame."""
import ctypes as C

import numpy as np
import pytest

import ao_ref
import oracle_lib as O
import raytracer as rt
from raytracer import _native as N

pytestmark = pytest.mark.gpu
SEED = 0x5EED
INF = float("inf")
W, H = 44, 28  # 6 x 4 tiles: the last tile column holds 4 pixel columns, the last tile row 4 pixel rows


def pinhole(width, height):
    cam = rt.CameraBuilder(width=width, aspect_ratio=(width, height), vfov=20.0, focal_length=1.0).build(
        rt.CameraPosition((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), focus_length=10.0))
    assert (cam.image_width, cam.image_height, cam.has_lens) == (width, height, 0)
    return cam


@pytest.fixture(scope="module")
def scene():
    sc = rt.scenes.random_scene(SEED).finalize(SEED)
    return sc, O.OracleScene(sc)


def settings(spp=2, **kw):
    return rt.RenderSettings(samples=spp, seed=SEED, **kw)


def check(got, ref, label):
    print(f"{label}: {ref.vertices} vertices ({ref.metal} metal, {ref.exhausted} chain-exhausted dielectric), "
          f"{ref.occluded} occluded, {ref.misses} misses")
    assert got.shape == ref.sums.shape
    assert np.array_equal(got, ref.sums), f"{label}: {int(np.sum(got != ref.sums))} pixels differ"


def test_cornell(gpu):
    sc = rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED)
    cam = rt.cornell_camera(40)
    gpu.upload(sc)
    ref = ao_ref.oracle_ao(sc, cam, SEED, 0, 2, 0, 300.0)
    check(gpu.render_ao(cam, settings(), chain=0, radius=300.0), ref, "cornell 40x40 radius 300")
    assert ref.occluded > 0 and ref.vertices - ref.occluded > 0 and ref.misses > 0


@pytest.mark.parametrize("radius", [0.5, INF])
def test_random_scene_pinhole(gpu, scene, radius):
    sc, osc = scene
    cam = pinhole(W, H)
    gpu.upload(sc)
    ref = ao_ref.oracle_ao(sc, cam, SEED, 0, 2, 8, radius, osc)
    check(gpu.render_ao(cam, settings(), chain=8, radius=radius), ref, f"random {W}x{H} pinhole radius {radius}")
    # every kind of vertex is in the frame: metal, a dielectric with the chain exhausted, misses, both answers
    assert ref.metal > 0 and ref.exhausted > 0 and ref.misses > 0
    assert ref.occluded > 0 and ref.vertices - ref.occluded > 0


def test_random_scene_lens_camera(gpu, scene):
    sc, osc = scene
    cam = rt.scene_camera("random", W, "std16x9")
    assert cam.has_lens and cam.image_width == W
    gpu.upload(sc)
    ref = ao_ref.oracle_ao(sc, cam, SEED, 0, 2, 8, 2.0, osc)
    assert ref.most_attempts > 1, "no sample of the frame rejected a lens-disk point: change the seed"
    check(gpu.render_ao(cam, settings(), chain=8, radius=2.0), ref, f"random {W}x{cam.image_height} lens radius 2")


def test_node_placements_give_identical_buffers(gpu, scene):
    sc, _ = scene
    cam = pinhole(W, H)
    res = []
    for nodes in ("global", "lds", "auto"):
        gpu.upload(sc, nodes=nodes)
        res.append(gpu.render_ao(cam, settings(), chain=8, radius=0.5))
    gpu.upload(sc)
    assert np.any(res[0] != res[0].flat[0])
    for other in res[1:]:
        assert np.array_equal(res[0], other)


def test_sample_ranges_add_up(gpu, scene):
    sc, _ = scene
    cam = pinhole(W, H)
    gpu.upload(sc)
    full = gpu.render_ao(cam, settings(4), chain=8, radius=0.5)
    lo = gpu.render_ao(cam, settings(4, sample_begin=0, sample_count=2), chain=8, radius=0.5)
    hi = gpu.render_ao(cam, settings(4, sample_begin=2, sample_count=2), chain=8, radius=0.5)
    assert np.array_equal(lo, gpu.render_ao(cam, settings(2), chain=8, radius=0.5))
    assert not np.array_equal(lo, hi)
    assert np.array_equal(lo + hi, full)  # integer sums: exact
    assert np.array_equal(full, np.round(full)) and full.min() >= 0 and full.max() <= 4


def test_device_form_equals_the_host_copy(gpu, scene):
    import torch
    sc, _ = scene
    cam = pinhole(W, H)
    gpu.upload(sc)
    host = gpu.render_ao(cam, settings(), chain=8, radius=0.5)
    out = torch.full((H, W), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.render_ao_device(cam, settings(), 8, 0.5, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(host, out.cpu().numpy())


def test_book2_scene_is_unsupported_and_bad_arguments_are_invalid(gpu, scene):
    sc, _ = scene
    cam = pinhole(W, H)
    gpu.upload(rt.scenes.final_scene(SEED, 4, 30).finalize(SEED))
    with pytest.raises(rt.RtError) as e:
        gpu.render_ao(cam, settings(), chain=0, radius=1.0)
    assert e.value.code == N.RT_E_UNSUPPORTED
    gpu.upload(sc)
    bad = [dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=-INF), dict(chain=-1),
           dict(tile_world=2), dict(sample_begin=3, sample_count=2)]
    for kw in bad:
        chain, radius = kw.pop("chain", 0), kw.pop("radius", 1.0)
        with pytest.raises(rt.RtError) as e:
            gpu.render_ao(cam, settings(4, **kw), chain=chain, radius=radius)
        assert e.value.code == N.RT_E_INVALID, (kw, chain, radius)
    p = settings().params()
    assert N.rt_lib().rt_render_ao(gpu.handle, C.byref(cam), C.byref(p), 0, 1.0, None) == N.RT_E_INVALID
