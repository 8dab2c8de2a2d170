"""The visibility-aware light pick on the device (rt_scene_light_visibility, rt_light_visibility_masks;
lightvis.hip; include/shirley_rt.h) against the restatement of its definition
(tests/lightvis_ref.py): the masks the kernel traced, the rows in force, the report, and rt_render_nee /
rt_render_direct with those rows.  The kernel's shadow rays go through the any-hit walk the passes use, the rows
are built with + - * /, and the passes only read other numbers, so wherever no vertex albedo needs a libm function
every comparison is exact equality."""
import math

import numpy as np
import pytest

import direct_ref as D
import lightgrid_ref as G
import lightvis_ref as V
import oracle_lib as O
import raytracer as rt
import rect_ref as RR
from raytracer import _native as N
from raytracer import scene as S

pytestmark = pytest.mark.gpu
SEED = 0x5EED
HW, HH = 20, 12
MIS = [False, True]
ALL = N.RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL if hasattr(N, "RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL") else 3


def settings(spp=4, depth=4, **kw):
    return rt.RenderSettings(samples=spp, max_reflect=depth, seed=SEED, **kw)


@pytest.fixture(autouse=True)
def uniform_again(gpu):
    """The context is the session's: leave it with the uniform pick and area sampling, whatever the test did."""
    yield
    try:
        gpu.light_pick(0)
        gpu.light_sampling(N.RT_LIGHT_SAMPLE_AREA)
    except rt.RtError:  # (no scene uploaded yet)
        pass


class Case:
    """A scene, its oracle, its light list and plain grid, and the restatement's masks per K (computed on demand,
    once)."""

    def __init__(self, sc, cells):
        self.sc, self.cells, self.osc = sc, cells, O.OracleScene(sc)
        self.lights, _ = D.list_lights(sc.desc)
        self.grid = G.Grid(self.lights, cells)
        self._masks = {}

    def masks(self, rays):
        if rays not in self._masks:
            self._masks[rays] = V.Masks(self.grid, self.lights, self.osc, rays, SEED)
        return self._masks[rays]

    def vis_grid(self, rays):
        return V.grid_with(self.grid, V.rows(self.grid, self.lights, self.masks(rays).masks, rays))

    def set(self, gpu, rays, **kw):
        gpu.upload(self.sc, **kw)
        gpu.light_pick(self.cells)
        return gpu.light_visibility(rays, SEED)


@pytest.fixture(scope="module")
def hand():
    return Case(D.hand_scene(extras=True).finalize(SEED), 3)


@pytest.fixture(scope="module")
def night():
    return Case(rt.scenes.random_scene(SEED, night=True).finalize(SEED), 8)


def popcount(a):
    return int(sum(bin(int(v)).count("1") for v in np.asarray(a).reshape(-1)))


# ---- the masks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rays", [1, 8, 32])
def test_hand_scene_masks_equal_the_oracles(gpu, hand, rays):
    """135 pairs: K = 1 puts 64 groups in a wave, K = 32 two; 135 * K is a multiple of 64 for no K here, so the last
    wave has idle lanes that stay for the ballot."""
    rep = hand.set(gpu, rays)
    want = hand.masks(rays)
    got = gpu.light_visibility_masks()
    assert got.size == 135 and (135 * rays) % 64 != 0
    assert np.array_equal(got.reshape(want.masks.shape), want.masks), f"{int(np.sum(got != want.masks.reshape(-1)))} masks"
    assert (rep.rays, rep.seed, rep.pairs) == (rays, SEED, 135)
    assert (rep.traced, rep.unoccluded, rep.dead_points) == (want.traced, want.unoccluded, want.dead_points)
    assert rep.kernel_ms > 0.0
    if rays == 8:
        assert want.no_ray > 0 and want.dead_points > 0 and 0 < want.unoccluded < want.traced


def test_night_random_masks_equal_the_oracles(gpu, night):
    rep = night.set(gpu, 8)
    want = night.masks(8)
    got = gpu.light_visibility_masks().reshape(want.masks.shape)
    print(f"night random 8 cells K 8: {want.masks.shape} masks, {want.traced} rays, {want.unoccluded} bits set, "
          f"{want.dead_points} dead points; kernel {rep.kernel_ms:.3f} ms")
    assert want.masks.shape[1] > 100 and want.traced > 70000
    assert np.array_equal(got, want.masks), f"{int(np.sum(got != want.masks))} masks differ"
    assert (rep.traced, rep.unoccluded, rep.dead_points) == (want.traced, want.unoccluded, want.dead_points)
    assert rep.pairs == want.masks.size


def test_night_random_masks_equal_the_projects_own_query(gpu, night):
    """rt_scene_occluded over rt_light_visibility_rays_host's rays gives the device's masks."""
    night.set(gpu, 8)
    got = gpu.light_visibility_masks()
    n_cells, L = night.masks(8).masks.shape
    rays = np.zeros((n_cells * L, 8, 6))
    traced = np.zeros((n_cells * L, 8), dtype=np.uint8)
    for c in range(n_cells):
        for j in range(L):
            rays[c * L + j], traced[c * L + j] = rt.light_visibility_rays_host(night.sc, 8, 8, SEED, c, j)
    occ = gpu.occluded(rays.reshape(-1, 6), D.T_MIN, D.T_MAX).reshape(-1, 8)
    bits = np.where(traced == 1, occ == 0, True)
    masks = (bits.astype(np.uint32) << np.arange(8, dtype=np.uint32)).sum(axis=1).astype(np.uint32)
    assert np.array_equal(masks, got)


@pytest.mark.parametrize("nodes,bvh", [("auto", "reference"), ("lds", "reference"), ("global", "reference"),
                                       ("half-lds", "reference"), ("auto", "sah"), ("global", "sah")])
def test_placements_and_builders_give_identical_masks(gpu, hand, nodes, bvh):
    hand.set(gpu, 8, bvh=bvh, nodes=nodes)
    got = gpu.light_visibility_masks()
    gpu.upload(hand.sc)
    assert np.array_equal(got, hand.masks(8).masks.reshape(-1)), (nodes, bvh)


# ---- the rows in force ------------------------------------------------------------------------------
def pick_points(grid):
    """The centre of every cell, and a point outside each of the box's six sides."""
    size = [(grid.hi[a] - grid.lo[a]) / float(grid.n[a]) for a in range(3)]
    pts = [[grid.lo[a] + (i[a] + 0.5) * size[a] for a in range(3)] for i in np.ndindex(*grid.n)]
    mid = [0.5 * (grid.lo[a] + grid.hi[a]) for a in range(3)]
    for a in range(3):
        for v in (grid.lo[a] - 7.0, grid.hi[a] + 7.0):
            pts.append([v if b == a else mid[b] for b in range(3)])
    return pts


def check_pick_at(gpu, grid):
    pts = pick_points(grid)
    assert {grid.cell(p) for p in pts} == set(range(len(grid.rows)))
    for xi in (0.0, 0.3, 0.77, math.nextafter(1.0, 0.0)):
        light, prob = gpu.light_pick_at(np.array(pts), np.full(len(pts), xi))
        want = [grid.pick(grid.cell(p), xi) for p in pts]
        assert light.tolist() == [k for k, _ in want] and prob.tolist() == [p for _, p in want], xi


def test_pick_at_reports_the_rows_built_from_the_device_masks(gpu, hand):
    hand.set(gpu, 8)
    cdf = rt.light_visibility_rows_host(hand.sc, 3, 8, gpu.light_visibility_masks())
    grid = V.grid_with(hand.grid, cdf.reshape(-1, 5).tolist())
    assert grid.rows != hand.grid.rows and grid.rows == hand.vis_grid(8).rows
    check_pick_at(gpu, grid)
    for row in grid.rows:  # the floor holds
        assert min(np.diff([0.0] + row)) >= 0.125 / 5 - 4e-16


# ---- exact frames -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mis", MIS)
def test_nee_on_the_hand_built_scene(gpu, hand, mis):
    cam = D.hand_camera(HW, HH)
    hand.set(gpu, 8)
    with V.visibility_rows(hand.vis_grid(8)):
        ref = G.oracle_nee(hand.sc, cam, SEED, 0, 4, 4, mis, 3, hand.osc)
    got = gpu.render_nee(cam, settings(), mis=mis)
    print(f"hand {HW}x{HH} cells 3 K 8 mis {mis}: {ref.counts()}")
    assert np.array_equal(got, ref.sums), f"{int(np.sum(got != ref.sums))} values differ"
    assert ref.cut > 0 and ref.occluded > 0 and ref.unoccluded > 0 and len(ref.kinds) == 5
    gpu.light_pick(3)
    assert not np.array_equal(gpu.render_nee(cam, settings(), mis=mis), got)  # (the new rows are in use)


def test_direct_on_the_hand_built_scene(gpu, hand):
    cam = D.hand_camera(HW, HH)
    hand.set(gpu, 8)
    with V.visibility_rows(hand.vis_grid(8)):
        ref = G.oracle_direct(hand.sc, cam, SEED, 0, 4, 2, 3, hand.osc)
    em, di = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=2)
    assert np.array_equal(em, ref.emission), f"{int(np.sum(em != ref.emission))} emission values differ"
    assert np.array_equal(di, ref.direct), f"{int(np.sum(di != ref.direct))} direct values differ"
    assert ref.occluded > 0 and ref.unoccluded > 0 and ref.direct.max() > 0.0


def test_nee_with_solid_angle_sampling_of_all_lights(gpu, hand):
    """The three settings are independent: the grid, the visibility rows and RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL."""
    cam = D.hand_camera(HW, HH)
    hand.set(gpu, 8)
    gpu.light_sampling(ALL)
    with V.visibility_rows(hand.vis_grid(8)):
        ref = RR.oracle_nee(hand.sc, cam, SEED, 0, 4, 4, True, 3, ALL, hand.osc)
    got = gpu.render_nee(cam, settings(), mis=True)
    bad = np.any(np.abs(got - ref.sums) > 1e-10 * 4, axis=-1)
    print(f"hand {HW}x{HH} cells 3 K 8, solid angle of all lights: {ref.counts()}; bit-identical channels "
          f"{np.mean(got == ref.sums):.5f}")
    assert ref.rect_angle > 0 and ref.unoccluded > 0
    assert np.array_equal(got, ref.sums), f"{int(np.sum(got != ref.sums))} values differ, {int(bad.sum())} pixels far"


@pytest.mark.parametrize("mis", MIS)
def test_night_random_scene_by_the_parity_criterion(gpu, night, mis):
    """tests/test_gpu_light_grid.py's night frame and criterion (exact equality where every vertex of the pixel has
    a solid albedo, elsewhere no channel further than 1e-10 * spp except in at most 0.1 % of pixels), with the
    visibility rows at 8 cells, K = 8."""
    spp = 2
    cam = rt.scene_camera("random", 48, "std16x9")
    night.set(gpu, 8)
    with V.visibility_rows(night.vis_grid(8)):
        ref = G.oracle_nee(night.sc, cam, SEED, 0, spp, 8, mis, 8, night.osc)
    got = gpu.render_nee(cam, settings(spp, 8), mis=mis)
    bad = np.any(np.abs(got - ref.sums) > 1e-10 * spp, axis=-1)
    print(f"night random {cam.image_width}x{cam.image_height} cells 8 K 8 mis {mis}: {ref.counts()}; "
          f"bit-identical channels {np.mean(got == ref.sums):.5f}, pixels beyond 1e-10 * spp {bad.mean():.5f}")
    assert ref.solid.any() and not ref.solid.all()
    assert ref.unoccluded > 0 and ref.occluded > 0
    assert np.array_equal(got[ref.solid], ref.sums[ref.solid])
    assert bad.mean() <= 0.001


def test_night_random_direct_by_the_parity_criterion(gpu, night):
    spp = 2
    cam = rt.scene_camera("random", 48, "std16x9")
    night.set(gpu, 8)
    with V.visibility_rows(night.vis_grid(8)):
        ref = G.oracle_direct(night.sc, cam, SEED, 0, spp, 8, 8, night.osc)
    em, di = gpu.render_direct(cam, rt.RenderSettings(samples=spp, seed=SEED), chain=8)
    bad = np.any(np.abs(di - ref.direct) > 1e-10 * spp, axis=-1)
    print(f"night random direct cells 8 K 8: cut {ref.cut}, occluded {ref.occluded}, unoccluded {ref.unoccluded}")
    assert np.array_equal(em[ref.solid], ref.emission[ref.solid])
    assert np.array_equal(di[ref.solid], ref.direct[ref.solid]) and bad.mean() <= 0.001
    assert ref.occluded > 0 and ref.unoccluded > 0


# ---- one light --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mis", MIS)
def test_cornell_box_equals_the_plain_grid(gpu, mis):
    """L = 1: every row is {1.0} whatever the masks."""
    sc = rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED)
    cam = rt.cornell_camera(24)
    gpu.upload(sc)
    gpu.light_pick(4)
    plain = gpu.render_nee(cam, settings(4, 6), mis=mis)
    em0, di0 = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=0)
    rep = gpu.light_visibility(8, SEED)
    masks = gpu.light_visibility_masks()
    assert rep.pairs == masks.size > 1 and rep.unoccluded == popcount(masks)
    assert plain.max() > 0.0 and np.array_equal(gpu.render_nee(cam, settings(4, 6), mis=mis), plain)
    em, di = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=0)
    assert di0.max() > 0.0 and np.array_equal(em, em0) and np.array_equal(di, di0)


# ---- expectation ------------------------------------------------------------------------------------
def boxed_lamp_field():
    """lightgrid_ref.lamp_field() with one Lambertian RectBox on the floor between the middle row's lamps: it hides
    lamps from the floor around it, so the visibility rows differ from the plain ones."""
    b = G.lamp_field()
    b.add(S.RectBox((-2.2, 0.0, -0.8), (-0.8, 1.1, 0.8)), S.Lambertian(S.TextureLoader.solid(0.6, 0.6, 0.6)))
    return b


def boxed32():
    return boxed_lamp_field().finalize(SEED), G.lamp_camera(32)


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


@pytest.mark.parametrize("mis", MIS)
def test_expectation_equals_the_megakernels_on_the_boxed_lamp_field(gpu, mis):
    """boxed_lamp_field() at 32x32 in K = 16 disjoint ranges of 16 spp, depth 4, 4 cells, visibility K = 8, against
    gpu.render at the same max_depth: each side's frame mean and its standard error from the K range means;
    |mean difference| <= 5 sqrt(se1^2 + se2^2), as in tests/test_gpu_light_grid.py.  The seed is fixed, so the test
    is deterministic.  The CPU restatement (lightgrid_ref.expectation_figures under lightvis_ref.visibility_rows
    against or_render_rows, the same seed, scene and ranges) measured, per sample:
      render 0.067255 +- 0.000583; MIS clear 0.066922 +- 0.000439 (|difference| 0.000333, bound 0.003648);
      MIS set 0.066970 +- 0.000468 (0.000285, bound 0.003738)
    Both sit within a tenth of their bound, so both flag values are asserted.  The grid is 4 x 1 x 4 (the lamps share
    one height), 1148 rays of 1152 bits are traced and 1033 bits are set.  The plain grid's restatement on the same
    ranges: MIS clear +- 0.000432, set +- 0.000459 — the cells lie at lamp height, above the box, so the rows barely
    move.  The visibility rows' standard error is printed beside the plain grid's, not asserted."""
    sc = boxed_lamp_field().finalize(SEED)
    cam = G.lamp_camera(32)
    gpu.upload(sc)
    assert len(gpu.lights()[0]) == 9 and gpu.lights()[1] == 0
    gpu.light_pick(4)
    _, _, se_plain = expectation(gpu, cam, 4, mis)
    rep = gpu.light_visibility(8, SEED)
    assert 0 < rep.unoccluded < rep.traced  # (the box and the occluders hide lamps from some cells)
    diff, bound, se_vis = expectation(gpu, cam, 4, mis)
    print(f"boxed lamp field mis {mis}: standard error per sample, visibility rows {se_vis:.6f}, plain grid "
          f"{se_plain:.6f}")
    assert diff <= bound


# ---- off means off ----------------------------------------------------------------------------------
def test_off_means_off(gpu, hand):
    cam = D.hand_camera(HW, HH)
    gpu.upload(hand.sc)
    gpu.light_pick(3)
    plain = gpu.render_nee(cam, settings(), mis=True)
    em0, di0 = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=2)

    def is_plain():
        check_pick_at(gpu, hand.grid)
        em, di = gpu.render_direct(cam, rt.RenderSettings(samples=4, seed=SEED), chain=2)
        with pytest.raises(rt.RtError) as e:  # no masks are in force
            gpu.light_visibility_masks()
        return (e.value.code == N.RT_E_INVALID and np.array_equal(gpu.render_nee(cam, settings(), mis=True), plain)
                and np.array_equal(em, em0) and np.array_equal(di, di0))

    assert is_plain()
    gpu.light_visibility(8, SEED)
    vis = gpu.render_nee(cam, settings(), mis=True)
    assert not np.array_equal(vis, plain)
    gpu.light_pick(3)  # the pick again: the plain rows
    assert is_plain()
    gpu.light_visibility(8, SEED)
    assert np.array_equal(gpu.render_nee(cam, settings(), mis=True), vis)
    rep = gpu.light_visibility(0, SEED)  # rays = 0
    assert (rep.rays, rep.pairs, rep.traced) == (0, 0, 0) and is_plain()
    gpu.light_visibility(32, SEED)
    gpu.light_visibility(8, SEED)  # a later setting replaces the earlier one
    assert np.array_equal(gpu.render_nee(cam, settings(), mis=True), vis)
    gpu.upload(hand.sc)  # an upload: the uniform pick, no rows at all
    uniform = gpu.render_nee(cam, settings(), mis=True)
    gpu.light_pick(3)
    assert is_plain() and not np.array_equal(uniform, plain)


def test_a_context_that_never_sets_it_renders_the_plain_grids_frames(gpu, hand):
    """tests/test_gpu_light_grid.py's reference for the plain grid (the parent's frames) still holds."""
    cam = D.hand_camera(HW, HH)
    gpu.upload(hand.sc)
    gpu.light_pick(3)
    ref = G.oracle_nee(hand.sc, cam, SEED, 0, 4, 4, True, 3, hand.osc)
    assert np.array_equal(gpu.render_nee(cam, settings(), mis=True), ref.sums)


# ---- status codes -----------------------------------------------------------------------------------
def test_status_codes(gpu, hand):
    fresh = rt.Device(0)
    try:
        with pytest.raises(rt.RtError) as e:  # before any upload
            fresh.light_visibility(8, SEED)
        assert e.value.code == N.RT_E_INVALID
    finally:
        fresh.close()
    gpu.upload(hand.sc)
    with pytest.raises(rt.RtError) as e:  # the uniform pick: no grid
        gpu.light_visibility(8, SEED)
    assert e.value.code == N.RT_E_INVALID
    gpu.light_pick(3)
    for rays in (3, 64, -1):
        with pytest.raises(rt.RtError) as e:
            gpu.light_visibility(rays, SEED)
        assert e.value.code == N.RT_E_INVALID, rays
    gpu.light_visibility(8, SEED)
    with pytest.raises(rt.RtError):  # a refused setting leaves the one in force
        gpu.light_visibility(3, SEED)
    assert np.array_equal(gpu.light_visibility_masks(), hand.masks(8).masks.reshape(-1))
    assert N.rt_lib().rt_light_visibility_masks(gpu.handle, None) == N.RT_E_INVALID
    gpu.upload(rt.scenes.random_scene(SEED).finalize(SEED))  # no listed light
    gpu.light_pick(4)
    with pytest.raises(rt.RtError) as e:
        gpu.light_visibility(8, SEED)
    assert e.value.code == N.RT_E_INVALID
    gpu.upload(rt.scenes.final_scene(SEED, 4, 30).finalize(SEED))  # book-2 objects
    gpu.light_pick(4)
    with pytest.raises(rt.RtError) as e:
        gpu.light_visibility(8, SEED)
    assert e.value.code == N.RT_E_UNSUPPORTED
