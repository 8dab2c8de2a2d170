"""Solid-angle sampling of sphere lights on the device (rt_scene_light_sampling, rt_light_sample_at; light_cone.h,
direct.h, nee.hip, direct.hip; include/shirley_rt.h) against the restatement of its definition
(tests/cone_ref.py): the light sample alone, then rt_render_nee and rt_render_direct with it.  Only + - * /, a
correctly rounded sqrt, comparisons and selects, so wherever no vertex albedo needs a libm function every
comparison is exact equality."""
import math

import numpy as np
import pytest

import cone_ref as K
import direct_ref as D
import lightgrid_ref as G
import oracle_lib as O
import raytracer as rt
from raytracer import _native as N
from test_light_cone import SCENES, mismatches

pytestmark = pytest.mark.gpu
SEED = 0x5EED
HW, HH = 20, 12  # 3 x 2 tiles: the last tile column holds 4 pixel columns, the last tile row 4 pixel rows
MIS = [False, True]
CELLS = [0, 3]  # the uniform pick, the light grid
AREA, CONE = K.AREA, K.CONE


def settings(spp=4, depth=4, **kw):
    return rt.RenderSettings(samples=spp, max_reflect=depth, seed=SEED, **kw)


@pytest.fixture(autouse=True)
def area_and_uniform_again(gpu):
    """The context is the session's: leave it with area sampling and the uniform pick, whatever the test did."""
    yield
    try:
        gpu.light_sampling(AREA)
        gpu.light_pick(0)
    except rt.RtError:  # (no scene uploaded yet)
        pass


@pytest.fixture(scope="module")
def hand():
    sc = D.hand_scene(extras=True).finalize(SEED)
    return sc, O.OracleScene(sc)


@pytest.fixture(scope="module")
def hand_ref(hand):
    """The hand-built frame's restatements in mode SOLID_ANGLE, 20x12 @ 4 spp, depth 4, pinhole, per (cells, mis):
    computed once, shared, left unchanged."""
    sc, osc = hand
    return {(cells, mis): K.oracle_nee(sc, D.hand_camera(HW, HH), SEED, 0, 4, 4, mis, cells, CONE, osc)
            for cells in CELLS for mis in MIS}


def cone_on(gpu, sc, cells=0, **kw):
    gpu.upload(sc, **kw)
    gpu.light_pick(cells)
    gpu.light_sampling(CONE)


# ---- the light sample alone -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_sample_at_equals_the_restatement(gpu, name):
    """The CPU test's vertex set (tests/test_light_cone.py checks what it holds), both modes, both picks; then a
    batch of one lane and batches a wave less / plus one."""
    sc = SCENES[name]()
    lights, _ = D.list_lights(sc.desc)
    pts, nrm, _ = K.vertex_set(lights, SEED)
    gpu.upload(sc)
    for cells in CELLS:
        gpu.light_pick(cells)
        grid = G.Grid(lights, cells) if cells else None
        for mode in (AREA, CONE):
            gpu.light_sampling(mode)
            want = [K.record(grid, lights, mode, SEED, i, list(pts[i]), list(nrm[i])) for i in range(len(pts))]
            bad = mismatches(gpu.light_sample_at(pts, nrm, SEED), want)
            assert not bad, f"cells {cells} mode {mode}: {len(bad)} fields differ, first {bad[:3]}"
            for batch in (1, 63, 65):
                assert not mismatches(gpu.light_sample_at(pts[:batch], nrm[:batch], SEED), want[:batch]), batch
            assert (K.INSIDE in {w[1] for w in want}) == (mode == CONE)


# ---- exact frames -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("mis", MIS)
def test_nee_on_the_hand_built_scene(gpu, hand, hand_ref, cells, mis):
    sc, _ = hand
    cone_on(gpu, sc, cells)
    ref = hand_ref[(cells, mis)]
    got = gpu.render_nee(D.hand_camera(HW, HH), settings(), mis=mis)
    print(f"hand {HW}x{HH} cone cells {cells} mis {mis}: {ref.counts()}")
    assert np.array_equal(got, ref.sums), f"{int(np.sum(got != ref.sums))} values differ"
    sphere = sum(v for (geom, _), v in ref.kinds.items() if geom == N.RT_GEOM_SPHERE)
    assert sphere > 0 and len(ref.kinds) == 5 and ref.disk_rejects > 0 and ref.sphere_rejects == 0
    assert ref.reweighted_sphere_front > 0 and ref.reweighted_rect > 0
    assert ref.occluded > 0 and ref.unoccluded > 0 and ref.cut > 0
    gpu.light_sampling(AREA)
    assert not np.array_equal(gpu.render_nee(D.hand_camera(HW, HH), settings(), mis=mis), got)  # (the mode is in use)


@pytest.mark.parametrize("cells", CELLS)
def test_direct_on_the_hand_built_scene(gpu, hand, cells):
    sc, osc = hand
    cam = D.hand_camera(HW, HH)
    cone_on(gpu, sc, cells)
    ref = K.oracle_direct(sc, cam, SEED, 0, 4, 2, cells, CONE, osc)
    em, di = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=2)
    assert np.array_equal(em, ref.emission), f"{int(np.sum(em != ref.emission))} emission values differ"
    assert np.array_equal(di, ref.direct), f"{int(np.sum(di != ref.direct))} direct values differ"
    sphere = sum(v for (geom, _), v in ref.kinds.items() if geom == N.RT_GEOM_SPHERE)
    assert sphere > 0 and len(ref.kinds) == 5 and ref.occluded > 0 and ref.unoccluded > 0 and ref.chained > 0
    assert ref.direct.max() > 0.0


@pytest.mark.parametrize("w,h,spp,depth,begin", [(1, 1, 1, 1, 0), (9, 9, 1, 1, 0), (1, 1, 4, 4, 0), (9, 9, 5, 4, 3)])
@pytest.mark.parametrize("mis", MIS)
def test_small_shapes(gpu, hand, mis, w, h, spp, depth, begin):
    """One live lane in 64 (1x1), four tiles of which three are mostly empty (9x9), one sample of one segment (no
    light sample at all), and a range that starts at 3."""
    sc, osc = hand
    cam = D.hand_camera(w, h)
    cone_on(gpu, sc, 3)
    ref = K.oracle_nee(sc, cam, SEED, begin, spp, depth, mis, 3, CONE, osc)
    got = gpu.render_nee(cam, settings(spp, depth, sample_begin=begin, sample_count=spp - begin), mis=mis)
    assert np.array_equal(got, ref.sums), f"{int(np.sum(got != ref.sums))} values differ"
    dref = K.oracle_direct(sc, cam, SEED, begin, spp, 2, 3, CONE, osc)
    em, di = gpu.render_direct(cam, rt.RenderSettings(samples=spp, seed=SEED, sample_begin=begin,
                                                      sample_count=spp - begin), chain=2)
    assert np.array_equal(em, dref.emission) and np.array_equal(di, dref.direct)


@pytest.mark.parametrize("mis", MIS)
def test_sample_ranges_add_up(gpu, hand, hand_ref, mis):
    sc, _ = hand
    cam = D.hand_camera(HW, HH)
    cone_on(gpu, sc, 3)
    full = gpu.render_nee(cam, settings(4), mis=mis)
    assert np.array_equal(full, hand_ref[(3, mis)].sums)
    lo3 = gpu.render_nee(cam, settings(4, sample_begin=0, sample_count=3), mis=mis)
    hi1 = gpu.render_nee(cam, settings(4, sample_begin=3, sample_count=1), mis=mis)
    assert np.array_equal(lo3 + hi1, full) and not np.array_equal(lo3, full)


@pytest.mark.parametrize("nodes,bvh", [("auto", "reference"), ("lds", "reference"), ("global", "reference"),
                                       ("half-lds", "reference"), ("auto", "sah"), ("global", "sah")])
def test_placements_and_builders_give_identical_buffers(gpu, hand, hand_ref, nodes, bvh):
    sc, _ = hand
    cone_on(gpu, sc, 3, bvh=bvh, nodes=nodes)
    got = {mis: gpu.render_nee(D.hand_camera(HW, HH), settings(), mis=mis) for mis in MIS}
    gpu.upload(sc)
    for mis in MIS:
        assert np.array_equal(got[mis], hand_ref[(3, mis)].sums), (nodes, bvh, mis)


# ---- lifetime ---------------------------------------------------------------------------------------
def test_the_setting_lasts_until_the_next_upload(gpu, hand, hand_ref):
    sc, _ = hand
    cam = D.hand_camera(HW, HH)
    gpu.upload(sc)
    area = gpu.render_nee(cam, settings(), mis=True)  # before the setting was ever touched
    gpu.light_sampling(CONE)
    assert np.array_equal(gpu.render_nee(cam, settings(), mis=True), hand_ref[(0, True)].sums)
    gpu.light_pick(3)  # the pick and the mode are independent settings
    assert np.array_equal(gpu.render_nee(cam, settings(), mis=True), hand_ref[(3, True)].sums)
    gpu.light_pick(0)
    assert np.array_equal(gpu.render_nee(cam, settings(), mis=True), hand_ref[(0, True)].sums)
    gpu.upload(sc)  # resets the mode
    assert np.array_equal(gpu.render_nee(cam, settings(), mis=True), area)
    gpu.light_sampling(CONE)
    gpu.light_sampling(AREA)  # area sampling without an upload
    assert np.array_equal(gpu.render_nee(cam, settings(), mis=True), area)
    assert not np.array_equal(area, hand_ref[(0, True)].sums)


@pytest.mark.parametrize("mis", MIS)
def test_cornell_box_equals_area_sampling(gpu, mis):
    """One rect light and no sphere light: the mode changes nothing."""
    sc = rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED)
    cam = rt.cornell_camera(24)
    gpu.upload(sc)
    area = gpu.render_nee(cam, settings(4, 6), mis=mis)
    em0, di0 = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=0)
    gpu.light_sampling(CONE)
    assert area.max() > 0.0 and np.array_equal(gpu.render_nee(cam, settings(4, 6), mis=mis), area)
    em, di = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=0)
    assert di0.max() > 0.0 and np.array_equal(em, em0) and np.array_equal(di, di0)


def test_invalid_arguments_and_book2_scenes(gpu, hand):
    fresh = rt.Device(0)
    try:
        for call in (lambda: fresh.light_sampling(CONE), lambda: fresh.light_sample_at(np.zeros((1, 3)),
                                                                                       np.zeros((1, 3)), SEED)):
            with pytest.raises(rt.RtError) as e:  # before any upload
                call()
            assert e.value.code == N.RT_E_INVALID
    finally:
        fresh.close()
    sc, _ = hand
    cam = D.hand_camera(HW, HH)
    gpu.upload(sc)
    gpu.light_sampling(CONE)
    for mode in (-1, 2):
        with pytest.raises(rt.RtError) as e:
            gpu.light_sampling(mode)
        assert e.value.code == N.RT_E_INVALID, mode
    # a refused setting leaves the one in force
    one = gpu.light_sample_at(np.array([[2.5, 1.0, -1.0]]), np.array([[0.0, 1.0, 0.0]]), SEED)
    lights, _ = D.list_lights(sc.desc)
    assert not mismatches(one, [K.record(None, lights, CONE, SEED, 0, [2.5, 1.0, -1.0], [0.0, 1.0, 0.0])])
    assert len(gpu.light_sample_at(np.zeros((0, 3)), np.zeros((0, 3)), SEED)) == 0
    with pytest.raises(rt.RtError) as e:  # NULL buffers with n > 0
        rt.render._check(gpu.handle, N.rt_lib().rt_light_sample_at(gpu.handle, 1, None, None, SEED, None))
    assert e.value.code == N.RT_E_INVALID
    gpu.upload(rt.scenes.random_scene(SEED).finalize(SEED))  # lists no light
    with pytest.raises(rt.RtError) as e:
        gpu.light_sample_at(np.zeros((1, 3)), np.zeros((1, 3)), SEED)
    assert e.value.code == N.RT_E_INVALID
    gpu.upload(rt.scenes.final_scene(SEED, 4, 30).finalize(SEED))
    gpu.light_sampling(CONE)
    with pytest.raises(rt.RtError) as e:
        gpu.render_nee(cam, settings())
    assert e.value.code == N.RT_E_UNSUPPORTED
    with pytest.raises(rt.RtError) as e:
        gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=2)
    assert e.value.code == N.RT_E_UNSUPPORTED


# ---- night random -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [0, 8])
def test_night_random_scene_by_the_parity_criterion(gpu, cells):
    """tests/test_gpu_nee.py's criterion at its frame in mode SOLID_ANGLE: exact equality where every vertex of the
    pixel has a solid albedo, elsewhere no channel further than 1e-10 * spp except in at most 0.1 % of pixels
    (marble and checker albedos go through sin / floor).  The cone cuts fewer samples than the area form does on
    the same frame (both restatements' counts are printed): no sample lands on a lamp's far side."""
    spp, mis = 2, True
    sc = rt.scenes.random_scene(SEED, night=True).finalize(SEED)
    cam = rt.scene_camera("random", 48, "std16x9")
    cone_on(gpu, sc, cells)
    osc = O.OracleScene(sc)
    ref = K.oracle_nee(sc, cam, SEED, 0, spp, 8, mis, cells, CONE, osc)
    area = K.oracle_nee(sc, cam, SEED, 0, spp, 8, mis, cells, AREA, osc)
    got = gpu.render_nee(cam, settings(spp, 8), mis=mis)
    bad = np.any(np.abs(got - ref.sums) > 1e-10 * spp, axis=-1)
    print(f"night random {cam.image_width}x{cam.image_height} cone cells {cells}: {ref.counts()}; "
          f"{int(ref.solid.sum())} of {ref.solid.size} pixels solid; bit-identical channels "
          f"{np.mean(got == ref.sums):.5f}, pixels beyond 1e-10 * spp {bad.mean():.5f}")
    print(f"cut samples: cone {ref.cut} of {ref.sampled} (+ {ref.inside} from inside), area {area.cut} of "
          f"{area.sampled}")
    assert ref.solid.any() and not ref.solid.all(), "the frame must hold solid and textured albedos"
    assert ref.unoccluded > 0 and ref.occluded > 0 and ref.reweighted_sphere_front > 0
    assert np.array_equal(got[ref.solid], ref.sums[ref.solid])
    assert bad.mean() <= 0.001
    assert ref.cut < area.cut


# ---- expectation ------------------------------------------------------------------------------------
def expectation(gpu, cam, depth, mis, K_=16, n=16):
    a, b = [], []
    for k in range(K_):
        a.append(gpu.render_nee(cam, settings(K_ * n, depth, sample_begin=k * n, sample_count=n), mis=mis))
        b.append(gpu.render(cam, rt.RenderSettings(samples=K_ * n, max_reflect=depth, seed=SEED, sample_begin=k * n,
                                                   sample_count=n)))
    m1, s1 = D.range_means(a)
    m2, s2 = D.range_means(b)
    bound = 5.0 * math.sqrt(s1 * s1 + s2 * s2)
    print(f"depth {depth} mis {mis} per sample: nee {m1 / n:.6f} +- {s1 / n:.6f}, render {m2 / n:.6f} +- "
          f"{s2 / n:.6f}; |difference| {abs(m1 - m2) / n:.6f}, bound {bound / n:.6f}")
    assert s1 > 0.0 and s2 > 0.0 and m1 > 0.0
    return abs(m1 - m2), bound, s1 / n


@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("mis", MIS)
def test_expectation_equals_the_megakernels_on_the_lamp_field(gpu, depth, mis):
    """lightgrid_ref.lamp_field() (nine sphere lamps of unequal power over a floor, two occluders) at 32x32 in
    K = 16 disjoint ranges of 16 spp, uniform pick, mode SOLID_ANGLE, against gpu.render at the same max_depth: each
    side's frame mean and its standard error from the K range means; |mean difference| <= 5 sqrt(se1^2 + se2^2).
    The seed is fixed, so the test is deterministic.  The CPU restatement (cone_ref.expectation_figures against
    or_render_rows, the same seed, scene and ranges) measured, per sample:
      depth 2: render 0.067430 +- 0.000545; solid angle, MIS clear 0.067324 +- 0.000506 (|difference| 0.000106,
               bound 0.003718), MIS set 0.067332 +- 0.000501 (0.000098, bound 0.003701);
               area, MIS clear 0.067054 +- 0.000571, MIS set 0.067347 +- 0.000534
      depth 4: render 0.067577 +- 0.000542; solid angle, MIS clear 0.067489 +- 0.000505 (0.000088, bound 0.003705),
               MIS set 0.067498 +- 0.000500 (0.000079, bound 0.003687);
               area, MIS clear 0.067208 +- 0.000578, MIS set 0.067510 +- 0.000540
    Every solid-angle figure sits within half its bound, so both flag values are asserted at both depths.  The
    solid-angle mode's standard error is printed beside the area mode's, not asserted: on this frame most of either
    is the pick and the occluders, which the mode does not touch."""
    gpu.upload(G.lamp_field().finalize(SEED))
    cam = G.lamp_camera(32)
    assert len(gpu.lights()[0]) == 9 and gpu.lights()[1] == 0
    _, _, se_area = expectation(gpu, cam, depth, mis)
    gpu.light_sampling(CONE)
    diff, bound, se_cone = expectation(gpu, cam, depth, mis)
    print(f"lamp field depth {depth} mis {mis}: standard error per sample, solid angle {se_cone:.6f}, area "
          f"{se_area:.6f}")
    assert diff <= bound
