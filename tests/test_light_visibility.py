"""The visibility-aware light pick without a device (rt_light_visibility_rays_host, rt_light_visibility_rows_host;
scene_compile.cpp; include/shirley_rt.h) against the restatement of its definition
(tests/lightvis_ref.py): the rays of a pair and the rows for given masks, bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import direct_ref as D
import lightgrid_ref as G
import lightvis_ref as V
import oracle_lib as O
import raytracer as rt
from raytracer import _native as N

SEED = 0x5EED


def hand():
    """direct_ref's hand-built scene with its extras (an occluder and a glass sphere among the five lights), as
    tests/test_gpu_light_grid.py renders it: rects of all three orientations and two spheres."""
    return D.hand_scene(extras=True).finalize(SEED)


@pytest.fixture(scope="module")
def hand_masks():
    """The oracle's masks of the hand scene at 3 cells, K = 8: computed once, shared, left unchanged."""
    sc = hand()
    lights, _ = D.list_lights(sc.desc)
    grid = G.Grid(lights, 3)
    return sc, lights, grid, V.Masks(grid, lights, O.OracleScene(sc), 8, SEED)


def test_library_exports_the_symbols_within_abi_11():
    lib = N.rt_lib()
    for sym in ("rt_scene_light_visibility", "rt_light_visibility_masks", "rt_light_visibility_rays_host",
                "rt_light_visibility_rows_host"):
        assert sym in N.RT_SIGNATURES and getattr(lib, sym) is not None
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "shirley_rt.h")) as f:
        text = f.read()
    assert "#define RT_ABI_VERSION 11" in text
    assert "((double)u_j + 1.0) / ((double)Kc + 2.0)" in text  # the header states the rule the restatement follows
    assert C.sizeof(N.rt_light_visibility) == 56


def check_rays(sc, cells, rays):
    lights, _ = D.list_lights(sc.desc)
    grid = G.Grid(lights, cells)
    kinds, untraced = set(), 0
    for c in range(grid.n[0] * grid.n[1] * grid.n[2]):
        for j in range(len(lights)):
            got, traced = rt.light_visibility_rays_host(sc, cells, rays, SEED, c, j)
            kinds.add(lights[j][1])
            for i in range(rays):
                x, w, tr = V.ray(grid, lights, SEED, c, i, j)
                assert got[i].tolist() == x + w and bool(traced[i]) == tr, (c, j, i)
                untraced += not tr
    return grid, kinds, untraced


def test_rays_equal_the_restatement_on_the_hand_scene():
    grid, kinds, untraced = check_rays(hand(), 3, 4)
    assert grid.n == [3, 3, 3]
    assert kinds == {N.RT_GEOM_RECT_XY, N.RT_GEOM_RECT_YZ, N.RT_GEOM_RECT_XZ, N.RT_GEOM_SPHERE}
    # the points of a cell are shared by its lights, and a pair's draws do not depend on K
    sc = hand()
    a, _ = rt.light_visibility_rays_host(sc, 3, 4, SEED, 5, 0)
    b, _ = rt.light_visibility_rays_host(sc, 3, 4, SEED, 5, 3)
    k8, _ = rt.light_visibility_rays_host(sc, 3, 8, SEED, 5, 0)
    assert np.array_equal(a[:, :3], b[:, :3]) and np.array_equal(k8[:4], a)


def test_rays_equal_the_restatement_on_the_cornell_box():
    grid, kinds, _ = check_rays(rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED), 2, 4)
    assert max(grid.n) == 2 and min(grid.n) == 1 and kinds == {N.RT_GEOM_RECT_XZ}  # (a flat axis: size 0 there)


def test_the_hand_scene_inputs_are_worth_testing(hand_masks):
    """With the oracle alone: at 3 cells, K = 8 the masks hold a zero mask, a full one, a mixed one, a dead point
    and a bit decided without a ray."""
    _, _, _, M = hand_masks
    m = M.masks.reshape(-1)
    print(f"hand scene 3 cells K 8: {int((m == 0).sum())} zero, {int((m == 255).sum())} full, "
          f"{int(((m != 0) & (m != 255)).sum())} mixed masks; {M.dead_points} dead points, {M.no_ray} bits without "
          f"a ray, {M.traced} rays")
    assert (m == 0).any() and (m == 255).any() and ((m != 0) & (m != 255)).any()
    assert M.dead_points > 0 and M.no_ray > 0 and M.traced + M.no_ray == m.size * 8
    assert (m.size * 8) % 64 != 0  # (the device's last wave has idle lanes)


def test_rows_equal_the_restatement_given_the_oracles_masks(hand_masks):
    sc, lights, grid, M = hand_masks
    want = np.array(V.rows(grid, lights, M.masks, 8))
    got = rt.light_visibility_rows_host(sc, 3, 8, M.masks)
    assert got.shape == (3, 3, 3, 5) and np.array_equal(got.reshape(-1, 5), want)
    assert not np.array_equal(want, np.array(grid.rows))
    assert np.all(got[..., -1] == 1.0) and np.all(np.diff(got, axis=-1) > 0.0)


def test_all_ones_masks(hand_masks):
    """Every v_j = (K + 1) / (K + 2): the weights keep their ratios, the rows equal the plain ones up to rounding,
    and the library equals the restatement bit for bit."""
    sc, lights, grid, _ = hand_masks
    ones = np.full((27, 5), 0xFF, dtype=np.uint32)
    got = rt.light_visibility_rows_host(sc, 3, 8, ones).reshape(-1, 5)
    assert np.array_equal(got, np.array(V.rows(grid, lights, ones, 8)))
    assert np.allclose(got, np.array(grid.rows), rtol=0.0, atol=5 * 4 * 2.0 ** -53)  # (L terms of a few roundings)
    # bits at or above K are ignored
    high = np.full((27, 5), 0xFFFFFFFF, dtype=np.uint32)
    assert np.array_equal(rt.light_visibility_rows_host(sc, 3, 8, high).reshape(-1, 5), got)


def test_a_cell_without_a_live_point_keeps_the_plain_row(hand_masks):
    sc, lights, grid, M = hand_masks
    masks = M.masks.copy()
    masks[7, :] = 0  # Kc == 0
    masks[11, :] = 0xFFFFFF00  # ... and with bits above K only
    got = rt.light_visibility_rows_host(sc, 3, 8, masks).reshape(-1, 5)
    _, plain = rt.light_grid_host(sc, 3)
    plain = plain.reshape(-1, 5)
    assert np.array_equal(got[7], plain[7]) and np.array_equal(got[11], plain[11])
    assert np.array_equal(got, np.array(V.rows(grid, lights, masks, 8)))
    assert not np.array_equal(got[8], plain[8])


def test_a_light_no_point_sees_keeps_an_eighth_of_the_uniform_share(hand_masks):
    """u_j = 0 leaves v_j = 1 / (Kc + 2) > 0, so p_j stays above the floor 0.125 / L; with the other lights' weights
    far greater it comes down to the floor up to the running sum's rounding."""
    sc, lights, grid, _ = hand_masks
    for j in range(5):
        masks = np.full((27, 5), 0xFF, dtype=np.uint32)
        masks[:, j] = 0
        got = rt.light_visibility_rows_host(sc, 3, 8, masks).reshape(-1, 5)
        assert np.array_equal(got, np.array(V.rows(grid, lights, masks, 8)))
        p = np.diff(np.concatenate([np.zeros((27, 1)), got], axis=1), axis=1)
        plain = np.diff(np.concatenate([np.zeros((27, 1)), np.array(grid.rows)], axis=1), axis=1)
        assert np.all(p[:, j] >= 0.125 / 5 - 4e-16) and np.all(p[:, j] < plain[:, j])
    # a dark light that nothing sees: exactly the floor, up to the running sum's rounding
    sc = hand()  # (a scene of its own: the fixture's stays as it is)
    d = sc.desc
    t = d.textures[d.materials[d.objects[lights[2][0]].material].texture]
    for c in range(3):
        t.color[c] = 0.0
    masks = np.full((27, 5), 0xFF, dtype=np.uint32)
    masks[:, 2] = 0
    got = rt.light_visibility_rows_host(sc, 3, 8, masks).reshape(-1, 5)
    assert np.all(np.abs((got[:, 2] - got[:, 1]) - 0.125 / 5) <= 4e-16)


def test_invalid_arguments(hand_masks):
    sc, _, _, M = hand_masks
    lib = N.rt_lib()
    rays, traced, cdf = np.zeros((32, 6)), np.zeros(32, dtype=np.uint8), np.zeros(27 * 5)
    m = np.ascontiguousarray(M.masks)

    def rays_host(scene=sc.desc_ptr, cells=3, k=8, cell=0, light=0, out=rays.ctypes.data, tr=traced.ctypes.data):
        return lib.rt_light_visibility_rays_host(scene, cells, k, SEED, cell, light, out, tr)

    def rows_host(scene=sc.desc_ptr, cells=3, k=8, masks=m.ctypes.data, out=cdf.ctypes.data):
        return lib.rt_light_visibility_rows_host(scene, cells, k, masks, out)

    assert rays_host() == 0 and rows_host() == 0
    for k in (0, 3, 64, -1):
        assert rays_host(k=k) == N.RT_E_INVALID and rows_host(k=k) == N.RT_E_INVALID, k
    for cells in (0, -1, 65):
        assert rays_host(cells=cells) == N.RT_E_INVALID and rows_host(cells=cells) == N.RT_E_INVALID, cells
    assert rays_host(scene=None) == N.RT_E_INVALID and rows_host(scene=None) == N.RT_E_INVALID
    assert rays_host(out=None) == N.RT_E_INVALID and rays_host(tr=None) == N.RT_E_INVALID
    assert rows_host(masks=None) == N.RT_E_INVALID and rows_host(out=None) == N.RT_E_INVALID
    for cell, light in ((-1, 0), (27, 0), (0, -1), (0, 5)):
        assert rays_host(cell=cell, light=light) == N.RT_E_INVALID, (cell, light)
    assert rays_host(cell=26, light=4) == 0
    dark = rt.scenes.random_scene(SEED).finalize(SEED)  # no listed light
    assert rays_host(scene=dark.desc_ptr) == N.RT_E_INVALID and rows_host(scene=dark.desc_ptr) == N.RT_E_INVALID


# ---- ray-cli ----------------------------------------------------------------------------------------
CLI = os.path.join(N.BIN_DIR, "ray-cli")


def cli(*args):
    return subprocess.run([CLI, "render", "cornell", "-w", "64", "-s", "4"] + list(args), capture_output=True,
                          text=True, timeout=60)


def test_cli_lists_the_option():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--light-visibility K" in r.stderr


@pytest.mark.parametrize("args", [["--light-visibility", "8"], ["--light-visibility", "8", "--denoise"],
                                  ["--light-visibility", "8", "--nee"], ["--light-visibility", "8", "--direct"],
                                  ["--light-visibility", "8", "--nee", "--light-grid", "0"]])
def test_light_visibility_without_a_grid_and_a_pass_is_a_usage_error(args):
    """Refused with the usage text before a device is opened, like --light-grid."""
    r = cli(*args)
    assert r.returncode == 2
    assert "error: --light-visibility" in r.stderr and "usage: ray-cli" in r.stderr and "rt_create" not in r.stderr


@pytest.mark.parametrize("value", ["0", "3", "64", "-1"])
def test_a_bad_light_visibility_value_is_a_usage_error(value):
    r = cli("--nee", "--light-grid", "4", "--light-visibility", value)
    assert r.returncode == 2 and "--light-visibility K in 1, 2, 4, 8, 16, 32" in r.stderr
