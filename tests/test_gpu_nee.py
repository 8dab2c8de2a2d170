"""rt_render_nee (nee.hip; include/shirley_rt.h) against the CPU oracle's restatement of its
definition (tests/nee_ref.py), with RT_NEE_MIS clear and set.  A segment is the megakernel's own device code and
the weights are + - * /, a correctly rounded sqrt, comparisons and selects in a fixed order, so wherever no vertex
albedo needs a libm function every comparison is exact equality."""
import ctypes as C
import math

import numpy as np
import pytest

import direct_ref as D
import nee_ref as R
import oracle_lib as O
import raytracer as rt
from raytracer import _native as N

pytestmark = pytest.mark.gpu
SEED = 0x5EED
HW, HH = 20, 12  # 3 x 2 tiles: the last tile column holds 4 pixel columns, the last tile row 4 pixel rows
MIS = [False, True]


def settings(spp=4, depth=4, **kw):
    return rt.RenderSettings(samples=spp, max_reflect=depth, seed=SEED, **kw)


def check_exact(got, ref, label):
    print(f"{label}: {ref.counts()}")
    assert got.shape == ref.sums.shape
    assert np.array_equal(got, ref.sums), f"{label}: {int(np.sum(got != ref.sums))} values differ"


@pytest.fixture(scope="module")
def hand():
    sc = D.hand_scene(extras=True).finalize(SEED)
    return sc, O.OracleScene(sc)


@pytest.fixture(scope="module")
def hand_ref(hand):
    """The hand-built frame's restatement, 20x12 @ 4 spp, depth 4, pinhole, MIS clear and set: computed once,
    shared, left unchanged."""
    sc, osc = hand
    return {mis: R.oracle_nee(sc, D.hand_camera(HW, HH), SEED, 0, 4, 4, mis, osc) for mis in MIS}


@pytest.mark.parametrize("mis", MIS)
def test_cornell(gpu, mis):
    sc = rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED)
    cam = rt.cornell_camera(24)
    gpu.upload(sc)
    ref = R.oracle_nee(sc, cam, SEED, 0, 4, 6, mis)
    check_exact(gpu.render_nee(cam, settings(4, 6), mis=mis), ref, f"cornell 24x24 depth 6 mis {mis}")
    assert ref.solid.all()
    assert ref.cut > 0 and ref.occluded > 0 and ref.unoccluded > 0 and ref.reweighted > 0 and ref.depth_cut > 0
    assert ref.cut + ref.occluded + ref.unoccluded == ref.sampled and ref.longest == 6


@pytest.mark.parametrize("mis", MIS)
def test_hand_built_scene_pinhole(gpu, hand, hand_ref, mis):
    sc, _ = hand
    gpu.upload(sc)
    ref = hand_ref[mis]
    check_exact(gpu.render_nee(D.hand_camera(HW, HH), settings(), mis=mis), ref, f"hand {HW}x{HH} pinhole mis {mis}")
    # every light kind is sampled, spheres reject points, both kinds of listed hit are re-weighted, glass in view
    assert len(ref.kinds) == 5 and min(ref.kinds.values()) > 0 and ref.sphere_rejects > 0
    assert ref.reweighted_rect > 0 and ref.reweighted_sphere_front > 0
    assert ref.dielectric > 0 and ref.misses > 0
    assert ref.cut > 0 and ref.occluded > 0 and ref.unoccluded > 0


@pytest.mark.parametrize("mis", MIS)
def test_hand_built_scene_lens_camera(gpu, hand, mis):
    sc, osc = hand
    cam = D.hand_camera(HW, HH, aperture=0.25)
    gpu.upload(sc)
    ref = R.oracle_nee(sc, cam, SEED, 0, 4, 4, mis, osc)
    assert ref.most_attempts > 1, "no sample of the frame rejected a lens-disk point: change the seed"
    check_exact(gpu.render_nee(cam, settings(), mis=mis), ref, f"hand {HW}x{HH} lens mis {mis}")


@pytest.mark.parametrize("w,h,spp,depth,begin", [(1, 1, 4, 4, 0), (9, 9, 4, 4, 0), (9, 9, 1, 4, 0), (9, 9, 4, 1, 0),
                                                 (9, 9, 4, 2, 0), (9, 9, 5, 4, 2)])
@pytest.mark.parametrize("mis", MIS)
def test_small_shapes(gpu, hand, mis, w, h, spp, depth, begin):
    """One live lane in 64 (1x1), four tiles of which three are mostly empty (9x9), one sample, one and two
    segments, a range that starts past 0: where a wave-wide call or the loop's exit would go wrong."""
    sc, osc = hand
    cam = D.hand_camera(w, h)
    gpu.upload(sc)
    ref = R.oracle_nee(sc, cam, SEED, begin, spp, depth, mis, osc)
    got = gpu.render_nee(cam, settings(spp, depth, sample_begin=begin, sample_count=spp - begin), mis=mis)
    check_exact(got, ref, f"hand {w}x{h} @ [{begin}, {spp}) depth {depth} mis {mis}")
    assert ref.sums.max() > 0.0


@pytest.mark.parametrize("mis", MIS)
def test_sample_ranges_add_up(gpu, hand, hand_ref, mis):
    """A lane adds its samples in order into a running sum, so [0, S-1) + [S-1, S) equals [0, S) exactly (one more
    term added to the same partial sum) and a call over [0, k) holds the first k terms."""
    sc, _ = hand
    cam = D.hand_camera(HW, HH)
    gpu.upload(sc)
    full = gpu.render_nee(cam, settings(4), mis=mis)
    assert np.array_equal(full, hand_ref[mis].sums)
    lo3 = gpu.render_nee(cam, settings(4, sample_begin=0, sample_count=3), mis=mis)
    hi1 = gpu.render_nee(cam, settings(4, sample_begin=3, sample_count=1), mis=mis)
    lo2 = gpu.render_nee(cam, settings(4, sample_begin=0, sample_count=2), mis=mis)
    first2 = gpu.render_nee(cam, settings(2), mis=mis)
    assert np.array_equal(lo3 + hi1, full)
    assert np.array_equal(lo2, first2) and not np.array_equal(lo2, full)


@pytest.mark.parametrize("nodes,bvh", [("auto", "reference"), ("lds", "reference"), ("global", "reference"),
                                       ("half-lds", "reference"), ("auto", "sah"), ("global", "sah")])
def test_placements_and_builders_give_identical_buffers(gpu, hand, hand_ref, nodes, bvh):
    sc, _ = hand
    gpu.upload(sc, bvh=bvh, nodes=nodes)
    got = {mis: gpu.render_nee(D.hand_camera(HW, HH), settings(), mis=mis) for mis in MIS}
    gpu.upload(sc)
    for mis in MIS:
        assert np.array_equal(got[mis], hand_ref[mis].sums), (nodes, bvh, mis)


def test_device_form_equals_the_host_copy(gpu, hand, hand_ref):
    import torch
    sc, _ = hand
    cam = D.hand_camera(HW, HH)
    gpu.upload(sc)
    out = {mis: torch.full((HH, HW, 3), -1.0, dtype=torch.float64, device="cuda") for mis in MIS}
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    for mis in MIS:
        gpu.render_nee_device(cam, settings(), mis, out[mis].data_ptr(), stream)
    torch.cuda.synchronize()
    for mis in MIS:
        assert np.array_equal(out[mis].cpu().numpy(), hand_ref[mis].sums)


@pytest.mark.parametrize("mis", MIS)
def test_scene_without_a_listed_light_equals_the_megakernel(gpu, mis):
    """The day random scene lists no light: the integrator is the plain render, on the same device functions and
    the same streams as the megakernel, added in the same order."""
    sc = rt.scenes.random_scene(SEED).finalize(SEED)
    cam = rt.scene_camera("random", 16, "square")
    gpu.upload(sc)
    assert gpu.lights() == ([], 0)
    spp = 2
    want = gpu.render(cam, rt.RenderSettings(samples=spp, max_reflect=8, seed=SEED, sample_chunk=spp,
                                             engine="megakernel"))
    got = gpu.render_nee(cam, settings(spp, 8), mis=mis)
    assert want.max() > 0.0 and np.array_equal(got, want)


@pytest.mark.parametrize("mis", MIS)
def test_depth_1_equals_the_megakernel(gpu, mis):
    sc = D.lambert_box().finalize(SEED)
    cam = rt.default_camera(32, "square")
    gpu.upload(sc)
    spp = 4
    want = gpu.render(cam, rt.RenderSettings(samples=spp, max_reflect=1, seed=SEED, sample_chunk=spp,
                                             engine="megakernel"))
    got = gpu.render_nee(cam, settings(spp, 1), mis=mis)
    assert want.max() > 0.0 and np.array_equal(got, want)
    assert not gpu.render_nee(cam, settings(spp, 0), mis=mis).any()  # max_depth <= 0: zero sums


@pytest.mark.parametrize("mis", MIS)
def test_night_random_scene_by_the_parity_criterion(gpu, mis):
    """Marble (Perlin) and checker albedos go through sin / floor on the device and in the oracle: the project's
    parity criterion there (tests/test_gpu_parity.py: no channel further than 1e-10 * spp, except in at most
    PARITY_OUTLIERS = 0.1 % of pixels), exact equality where every vertex of the pixel has a solid albedo."""
    spp = 2
    sc = rt.scenes.random_scene(SEED, night=True).finalize(SEED)
    cam = rt.scene_camera("random", 48, "std16x9")
    gpu.upload(sc)
    assert len(gpu.lights()[0]) > 1
    ref = R.oracle_nee(sc, cam, SEED, 0, spp, 8, mis)
    got = gpu.render_nee(cam, settings(spp, 8), mis=mis)
    bad = np.any(np.abs(got - ref.sums) > 1e-10 * spp, axis=-1)
    print(f"night random {cam.image_width}x{cam.image_height} mis {mis}: {ref.counts()}; "
          f"{int(ref.solid.sum())} of {ref.solid.size} pixels solid; bit-identical channels "
          f"{np.mean(got == ref.sums):.5f}, pixels beyond 1e-10 * spp {bad.mean():.5f}")
    assert ref.solid.any() and not ref.solid.all(), "the frame must hold solid and textured albedos"
    assert ref.unoccluded > 0 and ref.occluded > 0 and ref.reweighted_sphere_front > 0
    assert np.array_equal(got[ref.solid], ref.sums[ref.solid])
    assert bad.mean() <= 0.001


def expectation(gpu, cam, depth, mis, K=16, n=16):
    a, b = [], []
    for k in range(K):
        a.append(gpu.render_nee(cam, settings(K * n, depth, sample_begin=k * n, sample_count=n), mis=mis))
        b.append(gpu.render(cam, rt.RenderSettings(samples=K * n, max_reflect=depth, seed=SEED, sample_begin=k * n,
                                                   sample_count=n)))
    m1, s1 = D.range_means(a)
    m2, s2 = D.range_means(b)
    bound = 5.0 * math.sqrt(s1 * s1 + s2 * s2)
    print(f"depth {depth} mis {mis} per sample: nee {m1 / n:.6f} +- {s1 / n:.6f}, render {m2 / n:.6f} +- "
          f"{s2 / n:.6f}; |difference| {abs(m1 - m2) / n:.6f}, bound {bound / n:.6f}")
    assert s1 > 0.0 and s2 > 0.0 and m1 > 0.0
    return abs(m1 - m2), bound


@pytest.mark.parametrize("depth", [2, 5])
@pytest.mark.parametrize("mis", MIS)
def test_expectation_equals_the_megakernels_on_the_lambert_box(gpu, depth, mis):
    """direct_ref.lambert_box() at 32x32 in K = 16 disjoint ranges of 16 spp against gpu.render at the same
    max_depth: each side's frame mean and its standard error from the K range means;
    |mean difference| <= 5 sqrt(se1^2 + se2^2).  The seed is fixed, so the test is deterministic.
    The CPU restatement (nee_ref.expectation_figures against or_render_rows, the same seed, scene and ranges)
    measured, per sample:
      depth 2: render 0.167289 +- 0.001170; MIS clear 0.167786 +- 0.001163 (|difference| 0.000497, bound 0.008247);
               MIS set 0.167837 +- 0.000383 (0.000548, bound 0.006155)
      depth 5: render 0.196941 +- 0.001186; MIS clear 0.195253 +- 0.001280 (0.001688, bound 0.008725);
               MIS set 0.196983 +- 0.000456 (0.000042, bound 0.006354)"""
    gpu.upload(D.lambert_box().finalize(SEED))
    cam = rt.default_camera(32, "square")
    assert (cam.image_width, cam.image_height) == (32, 32) and len(gpu.lights()[0]) == 2
    diff, bound = expectation(gpu, cam, depth, mis)
    assert diff <= bound


def test_expectation_equals_the_megakernels_on_the_cornell_box(gpu):
    """Cornell box 24x24, depth 6, K = 16 ranges of 16 spp, RT_NEE_MIS set: asserted as above.  RT_NEE_MIS clear is
    printed, not asserted: pure area sampling's 1 / distance^4 tail keeps the mean of a finite sample below the
    expectation until a rare huge weight arrives.  The CPU restatement measured, per sample:
    render 0.074616 +- 0.001774; MIS set 0.073050 +- 0.000616 (|difference| 0.001566, bound 0.009390);
    MIS clear 0.069318 +- 0.000306 (0.005298, 2.9 combined standard errors)."""
    gpu.upload(rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED))
    cam = rt.cornell_camera(24)
    expectation(gpu, cam, 6, False)  # (printed only)
    diff, bound = expectation(gpu, cam, 6, True)
    assert diff <= bound


def test_book2_scene_is_unsupported_and_bad_arguments_are_invalid(gpu, hand):
    sc, _ = hand
    cam = D.hand_camera(HW, HH)
    gpu.upload(rt.scenes.final_scene(SEED, 4, 30).finalize(SEED))
    with pytest.raises(rt.RtError) as e:
        gpu.render_nee(cam, settings())
    assert e.value.code == N.RT_E_UNSUPPORTED
    gpu.upload(sc)
    for kw in (dict(tile_world=2), dict(sample_begin=3, sample_count=2)):
        with pytest.raises(rt.RtError) as e:
            gpu.render_nee(cam, settings(4, **kw))
        assert e.value.code == N.RT_E_INVALID, kw
    p = settings().params()
    lib = N.rt_lib()
    buf = np.zeros((HH, HW, 3))
    for flags in (2, 3, -1, 1 << 16):  # unknown flag bits
        assert lib.rt_render_nee(gpu.handle, C.byref(cam), C.byref(p), flags, buf.ctypes.data) == N.RT_E_INVALID
    assert lib.rt_render_nee(gpu.handle, C.byref(cam), C.byref(p), 1, None) == N.RT_E_INVALID
    assert lib.rt_render_nee_device(gpu.handle, C.byref(cam), C.byref(p), 1, None, None) == N.RT_E_INVALID
