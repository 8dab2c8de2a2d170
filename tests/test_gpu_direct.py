"""rt_render_direct (direct.hip; include/shirley_rt.h) against the CPU oracle's restatement of its
definition (tests/direct_ref.py).  The estimator is + - * /, a correctly rounded sqrt, comparisons and selects in
a fixed order, so wherever the vertex albedo needs no libm function every comparison is exact equality."""
import ctypes as C
import math

import numpy as np
import pytest

import direct_ref as D
import oracle_lib as O
import raytracer as rt
from raytracer import _native as N

pytestmark = pytest.mark.gpu
SEED = 0x5EED
HW, HH = 20, 12  # 3 x 2 tiles: the last tile column holds 4 pixel columns, the last tile row 4 pixel rows


def settings(spp=4, **kw):
    return rt.RenderSettings(samples=spp, seed=SEED, **kw)


def counts(ref):
    return (f"{ref.sampled} light samples {ref.kinds}, {ref.cut} cut, {ref.occluded} occluded, {ref.unoccluded} "
            f"unoccluded, {ref.sphere_rejects} sphere rejections; {ref.diffuse_light} + {ref.fairy_light} emitter "
            f"vertices, {ref.misses} misses, {ref.chained} dielectric vertices followed")


def check_exact(got, ref, label):
    em, di = got
    print(f"{label}: {counts(ref)}")
    assert em.shape == ref.emission.shape and di.shape == ref.direct.shape
    assert np.array_equal(em, ref.emission), f"{label}: {int(np.sum(em != ref.emission))} emission values differ"
    assert np.array_equal(di, ref.direct), f"{label}: {int(np.sum(di != ref.direct))} direct values differ"


@pytest.fixture(scope="module")
def hand():
    sc = D.hand_scene(extras=True).finalize(SEED)
    return sc, O.OracleScene(sc)


@pytest.fixture(scope="module")
def hand_ref(hand):
    """The hand-built frame's restatement, 20x12 @ 4 spp, chain 2, pinhole: computed once, shared, left unchanged."""
    sc, osc = hand
    return D.oracle_direct(sc, D.hand_camera(HW, HH), SEED, 0, 4, 2, osc)


def test_cornell(gpu):
    sc = rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED)
    cam = rt.cornell_camera(24)
    gpu.upload(sc)
    lights, unlisted = gpu.lights()
    assert [(l.geometry, l.emitter, l.area) for l in lights] == [(N.RT_GEOM_RECT_XZ, N.RT_MAT_FAIRY_LIGHT, 13650.0)]
    assert unlisted == 0
    ref = D.oracle_direct(sc, cam, SEED, 0, 4, 0)
    check_exact(gpu.render_direct(cam, settings(), chain=0), ref, "cornell 24x24 chain 0")
    assert ref.cut > 0 and ref.occluded > 0 and ref.unoccluded > 0 and ref.fairy_light > 0 and ref.misses > 0


def test_hand_built_scene_pinhole(gpu, hand, hand_ref):
    sc, _ = hand
    gpu.upload(sc)
    lights, unlisted = gpu.lights()
    assert [(l.object, l.geometry, l.emitter, l.area, tuple(l.color)) for l in lights] == D.HAND_LIGHTS
    assert unlisted == D.HAND_UNLISTED
    ref = hand_ref
    check_exact(gpu.render_direct(D.hand_camera(HW, HH), settings(), chain=2), ref, f"hand {HW}x{HH} pinhole")
    # every light kind is sampled, both emitter kinds are seen, every outcome of a sample occurs
    assert len(ref.kinds) == 5 and min(ref.kinds.values()) > 0
    assert ref.diffuse_light > 0 and ref.fairy_light > 0 and ref.misses > 0 and ref.sphere_rejects > 0
    assert ref.cut > 0 and ref.occluded > 0 and ref.unoccluded > 0
    assert ref.chained > 0  # the glass sphere is in view


def test_hand_built_scene_lens_camera(gpu, hand):
    sc, osc = hand
    cam = D.hand_camera(HW, HH, aperture=0.25)
    gpu.upload(sc)
    ref = D.oracle_direct(sc, cam, SEED, 0, 4, 2, osc)
    assert ref.most_attempts > 1, "no sample of the frame rejected a lens-disk point: change the seed"
    check_exact(gpu.render_direct(cam, settings(), chain=2), ref, f"hand {HW}x{HH} lens")


def test_night_random_scene_within_the_libm_bound(gpu):
    """Marble (Perlin) and checker albedos go through sin / floor on the device and in the oracle: relative 1e-12
    (tests/test_gpu_parity.py's bound for u, v) there, exact where every vertex of the pixel has a solid albedo."""
    sc = rt.scenes.random_scene(SEED, night=True).finalize(SEED)
    cam = rt.scene_camera("random", 16, "square")
    assert (cam.image_width, cam.image_height) == (16, 16)
    gpu.upload(sc)
    ref = D.oracle_direct(sc, cam, SEED, 0, 2, 8)
    em, di = gpu.render_direct(cam, settings(2), chain=8)
    print(f"night random 16x16: {counts(ref)}; {int(ref.solid.sum())} of 256 pixels solid")
    assert ref.solid.any() and not ref.solid.all(), "the frame must hold solid and textured albedos"
    assert ref.unoccluded > 0 and ref.occluded > 0
    assert np.array_equal(em[ref.solid], ref.emission[ref.solid])
    assert np.array_equal(di[ref.solid], ref.direct[ref.solid])
    for got, want in ((em, ref.emission), (di, ref.direct)):
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))


@pytest.mark.parametrize("nodes,bvh", [("auto", "reference"), ("lds", "reference"), ("global", "reference"),
                                       ("half-lds", "reference"), ("auto", "sah"), ("global", "sah")])
def test_placements_and_builders_give_identical_buffers(gpu, hand, hand_ref, nodes, bvh):
    sc, _ = hand
    gpu.upload(sc, bvh=bvh, nodes=nodes)
    em, di = gpu.render_direct(D.hand_camera(HW, HH), settings(), chain=2)
    gpu.upload(sc)
    assert np.array_equal(em, hand_ref.emission) and np.array_equal(di, hand_ref.direct)


def test_sample_ranges_add_up(gpu, hand, hand_ref):
    """A lane adds its samples in order into a running sum, so a call over [0, k) holds the first k terms of the
    [0, S) sum exactly, and [0, S-1) + [S-1, S) equals [0, S) exactly (one more term added to the same partial
    sum).  [0, k) + [k, S) for S - k > 1 reassociates: equal within rounding only."""
    sc, _ = hand
    cam = D.hand_camera(HW, HH)
    gpu.upload(sc)
    full = gpu.render_direct(cam, settings(4), chain=2)
    assert np.array_equal(full[0], hand_ref.emission) and np.array_equal(full[1], hand_ref.direct)
    lo3 = gpu.render_direct(cam, settings(4, sample_begin=0, sample_count=3), chain=2)
    hi1 = gpu.render_direct(cam, settings(4, sample_begin=3, sample_count=1), chain=2)
    lo2 = gpu.render_direct(cam, settings(4, sample_begin=0, sample_count=2), chain=2)
    hi2 = gpu.render_direct(cam, settings(4, sample_begin=2, sample_count=2), chain=2)
    first2 = gpu.render_direct(cam, settings(2), chain=2)
    for k in (0, 1):
        assert np.array_equal(lo2[k], first2[k])
        assert np.array_equal(lo3[k] + hi1[k], full[k])
        assert not np.array_equal(lo2[k], hi2[k])
        assert np.allclose(lo2[k] + hi2[k], full[k], rtol=4 * np.finfo(float).eps, atol=0.0)


def test_device_form_equals_the_host_copy(gpu, hand, hand_ref):
    import torch
    sc, _ = hand
    cam = D.hand_camera(HW, HH)
    gpu.upload(sc)
    em = torch.full((HH, HW, 3), -1.0, dtype=torch.float64, device="cuda")
    di = torch.full((HH, HW, 3), -1.0, dtype=torch.float64, device="cuda")
    only = torch.full((HH, HW, 3), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    gpu.render_direct_device(cam, settings(), 2, em.data_ptr(), di.data_ptr(), stream)
    gpu.render_direct_device(cam, settings(), 2, 0, only.data_ptr(), stream)  # one output alone
    torch.cuda.synchronize()
    assert np.array_equal(em.cpu().numpy(), hand_ref.emission)
    assert np.array_equal(di.cpu().numpy(), hand_ref.direct)
    assert np.array_equal(only.cpu().numpy(), hand_ref.direct)


def test_scene_without_a_listed_light(gpu):
    """The day random scene lists no light: direct is 0 and emission is the sky the features pass reports as the
    albedo of a miss."""
    sc = rt.scenes.random_scene(SEED).finalize(SEED)
    cam = rt.scene_camera("random", 16, "square")
    gpu.upload(sc)
    assert gpu.lights() == ([], 0)
    em, di = gpu.render_direct(cam, settings(2), chain=8)
    ref = D.oracle_direct(sc, cam, SEED, 0, 2, 8)
    assert ref.sampled == 0 and ref.misses > 0
    assert not di.any() and not ref.direct.any()
    assert np.array_equal(em, ref.emission) and em.max() > 0.0


def test_book2_scene_is_unsupported_and_bad_arguments_are_invalid(gpu, hand):
    sc, _ = hand
    cam = D.hand_camera(HW, HH)
    gpu.upload(rt.scenes.final_scene(SEED, 4, 30).finalize(SEED))
    with pytest.raises(rt.RtError) as e:
        gpu.render_direct(cam, settings(), chain=0)
    assert e.value.code == N.RT_E_UNSUPPORTED
    gpu.upload(sc)
    for kw in (dict(chain=-1), dict(tile_world=2), dict(sample_begin=3, sample_count=2)):
        chain = kw.pop("chain", 0)
        with pytest.raises(rt.RtError) as e:
            gpu.render_direct(cam, settings(4, **kw), chain=chain)
        assert e.value.code == N.RT_E_INVALID, (kw, chain)
    p = settings().params()
    lib = N.rt_lib()
    assert lib.rt_render_direct(gpu.handle, C.byref(cam), C.byref(p), 0, None, None) == N.RT_E_INVALID
    assert lib.rt_render_direct_device(gpu.handle, C.byref(cam), C.byref(p), 0, None, None, None) == N.RT_E_INVALID


def test_expectation_equals_the_megakernels_two_segment_render(gpu):
    """The estimator's expectation.  direct_ref.lambert_box() holds Lambertian surfaces and listed lights only,
    sky NONE, so per pixel E[rt_render(max_depth = 2)] = E[emission + direct].  Both sides at 32x32 in K = 16
    disjoint sample ranges of 16 spp; each side's frame mean and its standard error from the K range means;
    |mean difference| <= 5 sqrt(se1^2 + se2^2).  The seed is fixed, so the test is deterministic.
    The CPU oracle (direct_ref.oracle_direct against or_render_rows, the same seed, scene and ranges) measured,
    per sample: emission + direct 0.166190 +- 0.000553, render 0.167289 +- 0.001170; |difference| 0.001099
    against the bound 0.006468 (0.85 of one combined standard error)."""
    sc = D.lambert_box().finalize(SEED)
    cam = rt.default_camera(32, "square")
    assert (cam.image_width, cam.image_height) == (32, 32)
    gpu.upload(sc)
    assert len(gpu.lights()[0]) == 2
    K, n = 16, 16
    a, b = [], []
    for k in range(K):
        em, di = gpu.render_direct(cam, settings(K * n, sample_begin=k * n, sample_count=n), chain=8)
        a.append(em + di)
        b.append(gpu.render(cam, rt.RenderSettings(samples=K * n, max_reflect=2, seed=SEED, sample_begin=k * n,
                                                   sample_count=n)))
    m1, s1 = D.range_means(a)
    m2, s2 = D.range_means(b)
    bound = 5.0 * math.sqrt(s1 * s1 + s2 * s2)
    print(f"per sample: emission + direct {m1 / n:.6f} +- {s1 / n:.6f}, render {m2 / n:.6f} +- {s2 / n:.6f}; "
          f"|difference| {abs(m1 - m2) / n:.6f}, bound {bound / n:.6f}")
    assert s1 > 0.0 and s2 > 0.0 and m1 > 0.0
    assert abs(m1 - m2) <= bound
