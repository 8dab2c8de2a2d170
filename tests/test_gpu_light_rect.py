"""Solid-angle sampling of rect lights on the device (rt_scene_light_sampling's third mode, rt_light_sample_at;
light_rect.h, direct.h, nee.hip, direct.hip; include/shirley_rt.h) against the restatement of its
definition (tests/rect_ref.py): the light sample alone, then rt_render_nee and rt_render_direct with it.  The
definition's sin, cos and acos are fixed sequences of IEEE operations, so wherever no vertex albedo needs a libm
function every comparison is exact equality."""
import math

import numpy as np
import pytest

import direct_ref as D
import lightgrid_ref as G
import oracle_lib as O
import raytracer as rt
import rect_ref as R
from raytracer import _native as N
from raytracer import scene as S
from test_light_cone import mismatches

pytestmark = pytest.mark.gpu
SEED = 0x5EED
HW, HH = 20, 12  # 3 x 2 tiles: the last tile column holds 4 pixel columns, the last tile row 4 pixel rows
DEPTH = 6
MIS = [False, True]
CELLS = [0, 3]  # the uniform pick, the light grid
AREA, CONE, ALL = R.AREA, R.CONE, R.ALL


def settings(spp=4, depth=DEPTH, **kw):
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


def hand_with_a_speck():
    """The hand-built scene plus a listed rect light 2^-8 on a side behind the others: from a vertex more than 4
    away its solid angle (2^-16 / distance^2 at most) is below 2^-20, so its sample there is the area form's."""
    b = D.hand_scene(extras=True)
    b.add(S.xy_rect(-3.0, -3.0 + 2.0 ** -8, 1.0, 1.0 + 2.0 ** -8, -3.75),
          S.DiffuseLight(S.TextureLoader.solid(9.0, 9.0, 9.0)))
    return b


FRAMES = {"hand": lambda: D.hand_scene(extras=True), "hand+speck": hand_with_a_speck}


@pytest.fixture(scope="module")
def frames():
    """name -> (scene, oracle scene, {(cells, mis): rt_render_nee's restatement in mode ALL at 20x12, 4 spp,
    depth 6}): computed once, shared, left unchanged."""
    out = {}
    for name in FRAMES:
        sc = FRAMES[name]().finalize(SEED)
        osc = O.OracleScene(sc)
        out[name] = sc, osc, {(cells, mis): R.oracle_nee(sc, D.hand_camera(HW, HH), SEED, 0, 4, DEPTH, mis, cells, ALL,
                                                          osc) for cells in CELLS for mis in MIS}
    return out


def select(gpu, sc, cells=0, mode=ALL, **kw):
    gpu.upload(sc, **kw)
    gpu.light_pick(cells)
    gpu.light_sampling(mode)


def parity(got, want, solid, spp):
    """tests/test_gpu_nee.py's criterion: exact equality where every vertex albedo of the pixel is solid; elsewhere
    no channel further than 1e-10 * spp, except in at most 0.1 % of pixels."""
    assert np.array_equal(got[solid], want[solid]), f"{int(np.sum(got[solid] != want[solid]))} solid values differ"
    bad = np.any(np.abs(got - want) > 1e-10 * spp, axis=-1)
    assert bad.mean() <= 0.001, f"{int(bad.sum())} pixels beyond 1e-10 * spp"


# ---- the light sample alone -------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", ["reference", "sah"])
def test_sample_at_equals_the_restatement(gpu, bvh):
    """The CPU test's 2000 vertices (tests/test_light_rect.py checks that they hold the definition's edges), both
    picks, both BVH builders; then a batch of one lane and batches a wave less / plus one."""
    sc = D.hand_scene(extras=True).finalize(SEED)
    lights, _ = D.list_lights(sc.desc)
    pts, nrm, _ = R.vertex_set(lights, SEED)
    gpu.upload(sc, bvh=bvh)
    for cells in CELLS:
        gpu.light_pick(cells)
        gpu.light_sampling(ALL)
        grid = G.Grid(lights, cells) if cells else None
        want = [R.record(grid, lights, ALL, SEED, i, list(pts[i]), list(nrm[i])) for i in range(len(pts))]
        bad = mismatches(gpu.light_sample_at(pts, nrm, SEED), want)
        assert not bad, f"cells {cells}: {len(bad)} fields differ, first {bad[:3]}"
        for batch in (1, 63, 65):
            assert not mismatches(gpu.light_sample_at(pts[:batch], nrm[:batch], SEED), want[:batch]), batch
        flags = {w[1] for w in want}
        assert {0, R.CUT, R.COPLANAR, R.SMALL} <= flags, flags


# ---- exact frames -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FRAMES))
@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("mis", MIS)
def test_nee_on_the_hand_built_scene(gpu, frames, name, cells, mis):
    sc, _, refs = frames[name]
    select(gpu, sc, cells)
    ref = refs[(cells, mis)]
    got = gpu.render_nee(D.hand_camera(HW, HH), settings(), mis=mis)
    print(f"{name} {HW}x{HH} mode 3 cells {cells} mis {mis}: {ref.counts()}; {ref.rect_angle} rect samples by solid "
          f"angle, {ref.fallback} by the area form, {ref.coplanar} coplanar; {int(ref.solid.sum())} of "
          f"{ref.solid.size} pixels solid")
    parity(got, ref.sums, ref.solid, 4)
    assert ref.solid.sum() > 200 and ref.rect_angle > 100 and ref.cut > 0 and ref.occluded > 0 and ref.unoccluded > 0
    assert ref.reweighted_rect > 0 and ref.reweighted_sphere_front > 0 and len(ref.kinds) == 5
    # the hand-built frame itself holds no rect below 2^-20 of the sky: the speck's frame stands for that case
    assert (ref.fallback > 0) == (name == "hand+speck")
    gpu.light_sampling(CONE)
    assert not np.array_equal(gpu.render_nee(D.hand_camera(HW, HH), settings(), mis=mis), got)  # (the mode is in use)


@pytest.mark.parametrize("name", sorted(FRAMES))
@pytest.mark.parametrize("cells", CELLS)
def test_direct_on_the_hand_built_scene(gpu, frames, name, cells):
    sc, osc, _ = frames[name]
    cam = D.hand_camera(HW, HH)
    select(gpu, sc, cells)
    ref = R.oracle_direct(sc, cam, SEED, 0, 4, 2, cells, ALL, osc)
    em, di = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=2)
    parity(em, ref.emission, ref.solid, 4)
    parity(di, ref.direct, ref.solid, 4)
    assert ref.rect_angle > 100 and ref.cut > 0 and ref.occluded > 0 and ref.unoccluded > 0 and ref.chained > 0
    assert (ref.fallback > 0) == (name == "hand+speck") and ref.direct.max() > 0.0


@pytest.mark.parametrize("nodes,bvh", [("lds", "reference"), ("global", "reference"), ("half-lds", "reference"),
                                       ("global", "sah")])
def test_placements_and_builders_give_identical_buffers(gpu, frames, nodes, bvh):
    sc, _, refs = frames["hand"]
    select(gpu, sc, 3, bvh=bvh, nodes=nodes)
    got = {mis: gpu.render_nee(D.hand_camera(HW, HH), settings(), mis=mis) for mis in MIS}
    gpu.upload(sc)
    for mis in MIS:
        parity(got[mis], refs[(3, mis)].sums, refs[(3, mis)].solid, 4)


@pytest.mark.parametrize("mis", MIS)
def test_cornell_box_equals_the_restatement_and_not_area_sampling(gpu, mis):
    """24x24, 4 spp, depth 6: every albedo is solid, so the frame equals the restatement bit for bit; one rect light,
    so it differs from the mode-0 frame (and mode 1's, which is mode 0's here)."""
    sc = rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED)
    cam = rt.cornell_camera(24)
    osc = O.OracleScene(sc)
    gpu.upload(sc)
    area = gpu.render_nee(cam, settings(4, 6), mis=mis)
    _, di0 = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=0)
    gpu.light_sampling(ALL)
    ref = R.oracle_nee(sc, cam, SEED, 0, 4, 6, mis, 0, ALL, osc)
    got = gpu.render_nee(cam, settings(4, 6), mis=mis)
    print(f"cornell 24x24 mode 3 mis {mis}: {ref.counts()}; {ref.rect_angle} by solid angle, {ref.coplanar} coplanar")
    assert ref.solid.all() and ref.rect_angle > 1000 and ref.reweighted_rect > 0
    assert np.array_equal(got, ref.sums), f"{int(np.sum(got != ref.sums))} values differ"
    assert not np.array_equal(got, area)
    dref = R.oracle_direct(sc, cam, SEED, 0, 4, 0, 0, ALL, osc)
    em, di = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=0)
    assert np.array_equal(em, dref.emission) and np.array_equal(di, dref.direct)
    assert di.max() > 0.0 and not np.array_equal(di, di0)


def test_lamp_field_equals_mode_one(gpu):
    """No light of the lamp field is a rect: mode 3's frames are mode 1's, byte for byte."""
    gpu.upload(G.lamp_field().finalize(SEED))
    cam = G.lamp_camera(32)
    frames = {}
    for mode in (CONE, ALL):
        gpu.light_sampling(mode)
        frames[mode] = [gpu.render_nee(cam, settings(4, 4), mis=mis) for mis in MIS]
        frames[mode] += list(gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=0))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(frames[CONE], frames[ALL]))
    assert all(a.max() > 0.0 for a in frames[ALL][:2]) and frames[ALL][3].max() > 0.0


# ---- lifetime ---------------------------------------------------------------------------------------
def test_the_setting_lasts_until_the_next_upload(gpu, frames):
    sc, _, refs = frames["hand"]
    cam = D.hand_camera(HW, HH)
    gpu.upload(sc)
    area = gpu.render_nee(cam, settings(), mis=True)  # before the setting was ever touched
    gpu.light_sampling(ALL)
    parity(gpu.render_nee(cam, settings(), mis=True), refs[(0, True)].sums, refs[(0, True)].solid, 4)
    gpu.light_pick(3)  # the pick and the mode are independent settings
    parity(gpu.render_nee(cam, settings(), mis=True), refs[(3, True)].sums, refs[(3, True)].solid, 4)
    gpu.light_pick(0)
    for mode in (2, 4, -1):  # a refused mode leaves the one in force
        with pytest.raises(rt.RtError) as e:
            gpu.light_sampling(mode)
        assert e.value.code == N.RT_E_INVALID, mode
    three = gpu.render_nee(cam, settings(), mis=True)
    parity(three, refs[(0, True)].sums, refs[(0, True)].solid, 4)
    gpu.upload(sc)  # resets the mode
    assert np.array_equal(gpu.render_nee(cam, settings(), mis=True), area)
    assert not np.array_equal(area, three)


def test_book2_scenes_stay_unsupported(gpu):
    cam = D.hand_camera(HW, HH)
    gpu.upload(rt.scenes.final_scene(SEED, 4, 30).finalize(SEED))
    gpu.light_sampling(ALL)
    with pytest.raises(rt.RtError) as e:
        gpu.render_nee(cam, settings())
    assert e.value.code == N.RT_E_UNSUPPORTED
    with pytest.raises(rt.RtError) as e:
        gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=2)
    assert e.value.code == N.RT_E_UNSUPPORTED


# ---- expectation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("mis", MIS)
def test_expectation_equals_the_megakernels_on_the_lambert_box(gpu, depth, mis):
    """direct_ref.lambert_box() (a rect light and a FairyLight sphere over Lambertian surfaces) at 16x16 in K = 16
    disjoint ranges of 16 spp, uniform pick, mode 3, against gpu.render at the same max_depth: each side's frame
    mean and its standard error from the K range means; |mean difference| <= 5 sqrt(se1^2 + se2^2).  The seed is
    fixed, so the test is deterministic.  The CPU restatement (rect_ref.expectation_figures against or_render_rows,
    the same seed, scene and ranges) measured, per sample:
      depth 2: render 0.165318 +- 0.002743; mode 3, MIS clear 0.168387 +- 0.000480 (|difference| 0.003069, bound
               0.013926), MIS set 0.168192 +- 0.000614 (0.002873, bound 0.014056);
               area, MIS clear 0.168800 +- 0.002157, MIS set 0.168319 +- 0.000749
      depth 4: render 0.192633 +- 0.002780; mode 3, MIS clear 0.195951 +- 0.000566 (0.003318, bound 0.014187),
               MIS set 0.195573 +- 0.000660 (0.002940, bound 0.014289);
               area, MIS clear 0.194620 +- 0.002114, MIS set 0.195577 +- 0.000872
    Every mode-3 figure sits within a quarter of its bound, so both flag values are asserted at both depths."""
    gpu.upload(D.lambert_box().finalize(SEED))
    cam = rt.default_camera(16, "square")
    gpu.light_sampling(ALL)
    K_, n = 16, 16
    a, b = [], []
    for k in range(K_):
        a.append(gpu.render_nee(cam, settings(K_ * n, depth, sample_begin=k * n, sample_count=n), mis=mis))
        b.append(gpu.render(cam, rt.RenderSettings(samples=K_ * n, max_reflect=depth, seed=SEED, sample_begin=k * n,
                                                   sample_count=n)))
    m1, s1 = D.range_means(a)
    m2, s2 = D.range_means(b)
    bound = 5.0 * math.sqrt(s1 * s1 + s2 * s2)
    print(f"lambert box depth {depth} mis {mis} per sample: nee mode 3 {m1 / n:.6f} +- {s1 / n:.6f}, render "
          f"{m2 / n:.6f} +- {s2 / n:.6f}; |difference| {abs(m1 - m2) / n:.6f}, bound {bound / n:.6f}")
    assert s1 > 0.0 and s2 > 0.0 and m1 > 0.0
    assert abs(m1 - m2) <= bound
