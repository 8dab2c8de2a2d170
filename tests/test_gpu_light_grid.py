"""The spatially weighted light pick on the device (rt_scene_light_pick, rt_light_pick_at; light_pick.h, direct.h,
nee.hip; include/shirley_rt.h) against the restatement of its definition (tests/lightgrid_ref.py):
the pick alone, then rt_render_nee and rt_render_direct with it.  The table is built with + - * /, the pick is a
search and a subtraction, and the passes are what tests/test_gpu_nee.py and test_gpu_direct.py check, so wherever
no vertex albedo needs a libm function every comparison is exact equality."""
import itertools
import math

import numpy as np
import pytest

import direct_ref as D
import lightgrid_ref as G
import nee_ref as R
import oracle_lib as O
import raytracer as rt
from raytracer import _native as N

pytestmark = pytest.mark.gpu
SEED = 0x5EED
HW, HH = 20, 12  # 3 x 2 tiles: the last tile column holds 4 pixel columns, the last tile row 4 pixel rows
MIS = [False, True]
CELLS = [1, 3]
INF, NAN = math.inf, math.nan


def settings(spp=4, depth=4, **kw):
    return rt.RenderSettings(samples=spp, max_reflect=depth, seed=SEED, **kw)


@pytest.fixture(autouse=True)
def uniform_again(gpu):
    """The context is the session's: leave it with the uniform pick, whatever the test did."""
    yield
    try:
        gpu.light_pick(0)
    except rt.RtError:  # (no scene uploaded yet)
        pass


@pytest.fixture(scope="module")
def hand():
    sc = D.hand_scene(extras=True).finalize(SEED)
    return sc, O.OracleScene(sc)


@pytest.fixture(scope="module")
def hand_ref(hand):
    """The hand-built frame's restatements, 20x12 @ 4 spp, depth 4, pinhole, per (cells, mis): computed once,
    shared, left unchanged."""
    sc, osc = hand
    return {(cells, mis): G.oracle_nee(sc, D.hand_camera(HW, HH), SEED, 0, 4, 4, mis, cells, osc)
            for cells in CELLS for mis in MIS}


# ---- the pick alone ---------------------------------------------------------------------------------
def pick_cases(grid):
    """(point, xi) pairs: every cell corner, every face exactly and one ulp to either side of it, a point outside
    each of the six sides, +-inf and NaN coordinates; with each point xi = 0, the largest double below 1, and every
    cdf value of the point's row with its two neighbours."""
    size = [(grid.hi[a] - grid.lo[a]) / float(grid.n[a]) for a in range(3)]
    faces = [[grid.lo[a] + float(i) * size[a] for i in range(grid.n[a])] + [grid.hi[a]] for a in range(3)]
    mid = [0.5 * (grid.lo[a] + grid.hi[a]) + 0.123 for a in range(3)]
    pts = [list(p) for p in itertools.product(*faces)]
    for a in range(3):
        for f in faces[a]:
            for v in (f, math.nextafter(f, -INF), math.nextafter(f, INF)):
                pts.append([v if b == a else mid[b] for b in range(3)])
        for v in (grid.lo[a] - 7.0, grid.hi[a] + 7.0, -INF, INF, NAN):
            pts.append([v if b == a else mid[b] for b in range(3)])
    pts.append([NAN, NAN, NAN])
    pts.append([INF, -INF, NAN])
    out = []
    for p in pts:
        row = grid.rows[grid.cell(p)]
        xis = [0.0, math.nextafter(1.0, 0.0)]
        for c in row:
            xis += [math.nextafter(c, 0.0), c, math.nextafter(c, 2.0)]
        out += [(p, xi) for xi in xis if xi < 1.0]  # (a draw is in [0, 1))
    return out


def test_pick_at_equals_the_restatement(gpu, hand):
    sc, _ = hand
    gpu.upload(sc)
    info = gpu.light_pick(3)
    grid = G.grid_of(sc.desc, 3)
    assert list(info.n) == grid.n and info.n_lights == 5 and max(grid.n) == 3 and min(grid.n) > 1
    assert list(info.lo) == grid.lo and list(info.hi) == grid.hi
    cases = pick_cases(grid)
    want = [grid.pick(grid.cell(p), xi) for p, xi in cases]
    cells_seen = {grid.cell(p) for p, _ in cases}
    assert len(cells_seen) == grid.n[0] * grid.n[1] * grid.n[2] and {k for k, _ in want} == set(range(5))
    assert len(cases) < 4096
    for batch in (1, 63, 64, 65, len(cases), 4096):  # one lane, a wave less / plus one, a whole grid of blocks
        sel = [cases[i % len(cases)] for i in range(batch)]
        light, prob = gpu.light_pick_at(np.array([p for p, _ in sel]), np.array([xi for _, xi in sel]))
        ref = [want[i % len(cases)] for i in range(batch)]
        assert light.tolist() == [k for k, _ in ref], batch
        assert prob.tolist() == [p for _, p in ref], batch
    assert all(p > 0.0 for _, p in want)


# ---- exact frames -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("mis", MIS)
def test_nee_on_the_hand_built_scene(gpu, hand, hand_ref, cells, mis):
    sc, _ = hand
    gpu.upload(sc)
    gpu.light_pick(cells)
    ref = hand_ref[(cells, mis)]
    got = gpu.render_nee(D.hand_camera(HW, HH), settings(), mis=mis)
    print(f"hand {HW}x{HH} cells {cells} mis {mis}: {ref.counts()}")
    assert np.array_equal(got, ref.sums), f"{int(np.sum(got != ref.sums))} values differ"
    assert len(ref.kinds) == 5 and min(ref.kinds.values()) > 0 and ref.sphere_rejects > 0
    assert ref.reweighted_rect > 0 and ref.reweighted_sphere_front > 0 and ref.dielectric > 0
    assert ref.cut > 0 and ref.occluded > 0 and ref.unoccluded > 0
    gpu.light_pick(0)
    uniform = gpu.render_nee(D.hand_camera(HW, HH), settings(), mis=mis)
    assert not np.array_equal(uniform, got)  # (the pick is in use)


@pytest.mark.parametrize("cells", CELLS)
def test_direct_on_the_hand_built_scene(gpu, hand, cells):
    sc, osc = hand
    cam = D.hand_camera(HW, HH)
    gpu.upload(sc)
    gpu.light_pick(cells)
    ref = G.oracle_direct(sc, cam, SEED, 0, 4, 2, cells, osc)
    em, di = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=2)
    assert np.array_equal(em, ref.emission), f"{int(np.sum(em != ref.emission))} emission values differ"
    assert np.array_equal(di, ref.direct), f"{int(np.sum(di != ref.direct))} direct values differ"
    assert len(ref.kinds) == 5 and ref.cut > 0 and ref.occluded > 0 and ref.unoccluded > 0 and ref.chained > 0
    assert ref.direct.max() > 0.0


@pytest.mark.parametrize("mis", MIS)
def test_sample_ranges_add_up(gpu, hand, hand_ref, mis):
    sc, _ = hand
    cam = D.hand_camera(HW, HH)
    gpu.upload(sc)
    gpu.light_pick(3)
    full = gpu.render_nee(cam, settings(4), mis=mis)
    assert np.array_equal(full, hand_ref[(3, mis)].sums)
    lo3 = gpu.render_nee(cam, settings(4, sample_begin=0, sample_count=3), mis=mis)
    hi1 = gpu.render_nee(cam, settings(4, sample_begin=3, sample_count=1), mis=mis)
    assert np.array_equal(lo3 + hi1, full) and not np.array_equal(lo3, full)


@pytest.mark.parametrize("nodes,bvh", [("auto", "reference"), ("lds", "reference"), ("global", "reference"),
                                       ("half-lds", "reference"), ("auto", "sah"), ("global", "sah")])
def test_placements_and_builders_give_identical_buffers(gpu, hand, hand_ref, nodes, bvh):
    sc, _ = hand
    gpu.upload(sc, bvh=bvh, nodes=nodes)
    gpu.light_pick(3)
    got = {mis: gpu.render_nee(D.hand_camera(HW, HH), settings(), mis=mis) for mis in MIS}
    gpu.upload(sc)
    for mis in MIS:
        assert np.array_equal(got[mis], hand_ref[(3, mis)].sums), (nodes, bvh, mis)


# ---- degenerate cases -------------------------------------------------------------------------------
@pytest.mark.parametrize("mis", MIS)
def test_cornell_box_equals_the_uniform_pick(gpu, mis):
    """L = 1: every row is {1.0}, p = 1.0, and area / 1.0 = area * 1.0 = area exactly."""
    sc = rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED)
    cam = rt.cornell_camera(24)
    gpu.upload(sc)
    uniform = gpu.render_nee(cam, settings(4, 6), mis=mis)
    em0, di0 = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=0)
    info = gpu.light_pick(4)
    assert info.n_lights == 1
    assert uniform.max() > 0.0 and np.array_equal(gpu.render_nee(cam, settings(4, 6), mis=mis), uniform)
    em, di = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=0)
    assert di0.max() > 0.0 and np.array_equal(em, em0) and np.array_equal(di, di0)


@pytest.mark.parametrize("mis", MIS)
def test_scene_without_a_listed_light_equals_the_megakernel(gpu, mis):
    sc = rt.scenes.random_scene(SEED).finalize(SEED)
    cam = rt.scene_camera("random", 16, "square")
    gpu.upload(sc)
    info = gpu.light_pick(4)
    assert info.n_lights == 0 and list(info.n) == [0, 0, 0]
    spp = 2
    want = gpu.render(cam, rt.RenderSettings(samples=spp, max_reflect=8, seed=SEED, sample_chunk=spp,
                                             engine="megakernel"))
    got = gpu.render_nee(cam, settings(spp, 8), mis=mis)
    assert want.max() > 0.0 and np.array_equal(got, want)
    with pytest.raises(rt.RtError) as e:  # nothing to pick from
        gpu.light_pick_at(np.zeros((1, 3)), np.zeros(1))
    assert e.value.code == N.RT_E_INVALID


# ---- lifetime ---------------------------------------------------------------------------------------
def test_the_setting_lasts_until_the_next_upload(gpu, hand, hand_ref):
    sc, _ = hand
    cam = D.hand_camera(HW, HH)
    gpu.upload(sc)
    uniform = gpu.render_nee(cam, settings(), mis=True)
    gpu.light_pick(3)
    assert np.array_equal(gpu.render_nee(cam, settings(), mis=True), hand_ref[(3, True)].sums)
    gpu.upload(sc)  # resets the pick
    assert np.array_equal(gpu.render_nee(cam, settings(), mis=True), uniform)
    with pytest.raises(rt.RtError) as e:  # ... and no grid is set
        gpu.light_pick_at(np.zeros((1, 3)), np.zeros(1))
    assert e.value.code == N.RT_E_INVALID
    gpu.light_pick(3)
    gpu.light_pick(1)  # a later setting replaces the earlier one
    assert np.array_equal(gpu.render_nee(cam, settings(), mis=True), hand_ref[(1, True)].sums)
    gpu.light_pick(0)  # the uniform pick without an upload
    assert np.array_equal(gpu.render_nee(cam, settings(), mis=True), uniform)
    assert not np.array_equal(uniform, hand_ref[(3, True)].sums)


def test_invalid_arguments(gpu, hand):
    fresh = rt.Device(0)
    try:
        with pytest.raises(rt.RtError) as e:  # before any upload
            fresh.light_pick(3)
        assert e.value.code == N.RT_E_INVALID
    finally:
        fresh.close()
    sc, _ = hand
    gpu.upload(sc)
    for cells in (-1, 65):
        with pytest.raises(rt.RtError) as e:
            gpu.light_pick(cells)
        assert e.value.code == N.RT_E_INVALID, cells
    gpu.light_pick(3)
    with pytest.raises(rt.RtError) as e:  # a refused setting leaves the one in force
        gpu.light_pick(65)
    light, prob = gpu.light_pick_at(np.zeros((1, 3)), np.zeros(1))
    assert 0 <= light[0] < 5 and prob[0] > 0.0
    assert gpu.light_pick_at(np.zeros((0, 3)), np.zeros(0))[0].size == 0


# ---- night random -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mis", MIS)
def test_night_random_scene_by_the_parity_criterion(gpu, mis):
    """tests/test_gpu_nee.py's criterion at its frame, with the grid pick at 8 cells: exact equality where every
    vertex of the pixel has a solid albedo, elsewhere no channel further than 1e-10 * spp except in at most
    PARITY_OUTLIERS = 0.1 % of pixels (marble and checker albedos go through sin / floor)."""
    spp = 2
    sc = rt.scenes.random_scene(SEED, night=True).finalize(SEED)
    cam = rt.scene_camera("random", 48, "std16x9")
    gpu.upload(sc)
    info = gpu.light_pick(8)
    assert info.n_lights == len(gpu.lights()[0]) > 100 and max(info.n) == 8
    ref = G.oracle_nee(sc, cam, SEED, 0, spp, 8, mis, 8)
    got = gpu.render_nee(cam, settings(spp, 8), mis=mis)
    bad = np.any(np.abs(got - ref.sums) > 1e-10 * spp, axis=-1)
    print(f"night random {cam.image_width}x{cam.image_height} cells 8 mis {mis}: {ref.counts()}; "
          f"{int(ref.solid.sum())} of {ref.solid.size} pixels solid; bit-identical channels "
          f"{np.mean(got == ref.sums):.5f}, pixels beyond 1e-10 * spp {bad.mean():.5f}")
    assert ref.solid.any() and not ref.solid.all(), "the frame must hold solid and textured albedos"
    assert ref.unoccluded > 0 and ref.occluded > 0 and ref.reweighted_sphere_front > 0
    assert np.array_equal(got[ref.solid], ref.sums[ref.solid])
    assert bad.mean() <= 0.001


# ---- expectation ------------------------------------------------------------------------------------
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
    return abs(m1 - m2), bound, s1 / n


@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("mis", MIS)
def test_expectation_equals_the_megakernels_on_the_lamp_field(gpu, depth, mis):
    """lightgrid_ref.lamp_field() (nine sphere lamps of unequal power over a floor, two occluders) at 32x32 in
    K = 16 disjoint ranges of 16 spp, 4 cells, against gpu.render at the same max_depth: each side's frame mean and
    its standard error from the K range means; |mean difference| <= 5 sqrt(se1^2 + se2^2).  The seed is fixed, so
    the test is deterministic.  The CPU restatement (lightgrid_ref.expectation_figures against or_render_rows, the
    same seed, scene and ranges) measured, per sample:
      depth 2: render 0.067430 +- 0.000545; MIS clear 0.067211 +- 0.000424 (|difference| 0.000219, bound 0.003451);
               MIS set 0.067250 +- 0.000446 (0.000180, bound 0.003518)
      depth 4: render 0.067577 +- 0.000542; MIS clear 0.067372 +- 0.000427 (0.000205, bound 0.003450);
               MIS set 0.067420 +- 0.000447 (0.000158, bound 0.003514)
    Both MIS clear figures sit within half their bound, so both flag values are asserted.  The uniform pick's
    restatement on the same ranges: depth 2 MIS clear +- 0.000571, set +- 0.000534; depth 4 +- 0.000578, +- 0.000540.
    The grid pick's standard error is printed beside the uniform pick's, not asserted."""
    gpu.upload(G.lamp_field().finalize(SEED))
    cam = G.lamp_camera(32)
    assert len(gpu.lights()) == 2 and len(gpu.lights()[0]) == 9 and gpu.lights()[1] == 0
    _, _, se_uniform = expectation(gpu, cam, depth, mis)
    info = gpu.light_pick(4)
    assert max(info.n) == 4
    diff, bound, se_grid = expectation(gpu, cam, depth, mis)
    print(f"lamp field depth {depth} mis {mis}: standard error per sample, grid pick {se_grid:.6f}, uniform pick "
          f"{se_uniform:.6f}")
    assert diff <= bound


@pytest.mark.parametrize("mis", MIS)
def test_expectation_equals_the_megakernels_on_the_lambert_box(gpu, mis):
    """direct_ref.lambert_box() at 32x32, depth 2, 4 cells: the two lights' box covers a corner of the frame, so
    most vertices clamp to a border cell.  As above; the CPU restatement measured, per sample:
    render 0.167289 +- 0.001170; MIS clear 0.167563 +- 0.001047 (|difference| 0.000274, bound 0.007850);
    MIS set 0.167829 +- 0.000364 (0.000540, bound 0.006125)."""
    gpu.upload(D.lambert_box().finalize(SEED))
    cam = rt.default_camera(32, "square")
    assert (cam.image_width, cam.image_height) == (32, 32) and len(gpu.lights()[0]) == 2
    gpu.light_pick(4)
    diff, bound, _ = expectation(gpu, cam, 2, mis)
    assert diff <= bound
