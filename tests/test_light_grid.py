"""The light grid of the spatially weighted light pick on the CPU (include/shirley_rt.h, added within ABI 11;
DESIGN.md §18): rt_light_grid_host against the restatement of the header's build (tests/lightgrid_ref.py) bit for
bit, the properties every row must have whatever the colours, the refusals, and ray-cli's --light-grid."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import direct_ref as D
import lightgrid_ref as G
import raytracer as rt
from raytracer import _native as N

CLI = os.path.join(N.BIN_DIR, "ray-cli")
SEED = 0x5EED
ULP1 = 2.0 ** -52  # an ulp of 1.0: no entry of a row is larger


def check_parity(scene, cells):
    info, cdf = rt.light_grid_host(scene, cells)
    ref = G.grid_of(scene.desc, cells)
    assert list(info.n) == ref.n and info.n_lights == ref.n_lights
    assert list(info.lo) == ref.lo and list(info.hi) == ref.hi
    assert cdf.shape == (ref.n[2], ref.n[1], ref.n[0], ref.n_lights)
    if ref.n_lights:
        assert np.array_equal(cdf, ref.cdf())
    return info, cdf


def check_rows(cdf):
    """Strictly increasing, ending in exactly 1.0, every increment >= 0.125 / L less a few ulps of 1.0."""
    L = cdf.shape[-1]
    rows = cdf.reshape(-1, L)
    assert not np.isnan(rows).any()
    assert np.all(rows[:, -1] == 1.0)
    inc = np.diff(np.concatenate([np.zeros((len(rows), 1)), rows], axis=1), axis=1)
    assert np.all(inc > 0.0)
    assert inc.min() >= 0.125 / L - 4.0 * ULP1, inc.min()


def test_library_exports_the_symbols_within_abi_11():
    lib = N.rt_lib()
    for sym in ("rt_light_grid_host", "rt_scene_light_pick", "rt_light_pick_at"):
        assert sym in N.RT_SIGNATURES and getattr(lib, sym) is not None
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "shirley_rt.h")) as f:
        text = f.read()
    assert "#define RT_ABI_VERSION 11" in text
    assert "0.875" in text and "0.125" in text  # the header states the two shares the restatement follows
    assert (G.WEIGHTED, G.UNIFORM) == (0.875, 0.125)


@pytest.mark.parametrize("cells", [1, 2, 5])
def test_hand_scene_table_equals_the_restatement(cells):
    """Five lights, every geometry and emitter kind; the box is flat on no axis, so every axis has cells."""
    sc = D.hand_scene().finalize(SEED)
    info, cdf = check_parity(sc, cells)
    assert info.n_lights == 5 and max(info.n) == cells and (cells == 1) == (cdf.size == 5)
    check_rows(cdf)
    # the rows depend on the cell once a cell's diagonal is shorter than the distances (at 2 cells it is not:
    # every light lies within a diagonal of every cell, and max(D2, rho2 + diag2) makes the eight rows one)
    assert (len({tuple(r) for r in cdf.reshape(-1, 5)}) > 1) == (cells == 5)


def test_night_random_table_equals_the_restatement():
    sc = rt.scenes.random_scene(SEED, night=True).finalize(SEED)
    info, cdf = check_parity(sc, 8)
    assert info.n_lights == len(D.list_lights(sc.desc)[0]) > 100 and max(info.n) == 8
    check_rows(cdf)


def test_cornell_box_has_one_light_and_every_entry_is_one():
    sc = rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED)
    info, cdf = check_parity(sc, 4)
    assert info.n_lights == 1 and min(info.n) == 1 and cdf.size == info.n[0] * info.n[1] * info.n[2]
    assert np.all(cdf == 1.0)


def test_scene_without_a_listed_light_writes_no_table():
    sc = rt.scenes.random_scene(SEED).finalize(SEED)
    info, cdf = check_parity(sc, 4)
    assert info.n_lights == 0 and list(info.n) == [0, 0, 0] and cdf.size == 0
    guard = np.full(8, -7.0)
    got = N.rt_light_grid()
    assert N.rt_lib().rt_light_grid_host(sc.desc_ptr, 4, C.byref(got), guard.ctypes.data) == 0
    assert got.n_lights == 0 and np.all(guard == -7.0)


HOSTILE = [0.0, -3.0, math.inf, math.nan, 1e308]


@pytest.mark.parametrize("cells", [1, 3])
@pytest.mark.parametrize("shift", range(len(HOSTILE)))
def test_hostile_colours_leave_every_row_a_distribution(cells, shift):
    """Solid colours 0, negative, inf, NaN and 1e308 mixed into the hand scene's five lights, in five rotations:
    no entry is a NaN, the row properties hold, and the table still equals the restatement."""
    sc = D.hand_scene().finalize(SEED)
    d = sc.desc
    lights, _ = D.list_lights(d)
    for j, l in enumerate(lights):
        t = d.textures[d.materials[d.objects[l[0]].material].texture]
        t.color[j % 3] = HOSTILE[(j + shift) % len(HOSTILE)]
    _, cdf = check_parity(sc, cells)
    check_rows(cdf)


def test_all_dark_lights_give_the_uniform_row():
    sc = D.hand_scene().finalize(SEED)
    d = sc.desc
    for l in D.list_lights(d)[0]:
        t = d.textures[d.materials[d.objects[l[0]].material].texture]
        for c in range(3):
            t.color[c] = 0.0
    _, cdf = check_parity(sc, 2)
    assert np.all(cdf.reshape(-1, 5) == np.array([0.2, 0.4, 0.6, 0.8, 1.0]))


def test_invalid_arguments():
    lib = N.rt_lib()
    sc = D.hand_scene().finalize(SEED)
    info = N.rt_light_grid()
    for cells in (-1, 0, 65):
        assert lib.rt_light_grid_host(sc.desc_ptr, cells, C.byref(info), None) == N.RT_E_INVALID, cells
        with pytest.raises(rt.RtError) as e:
            rt.light_grid_host(sc, cells)
        assert e.value.code == N.RT_E_INVALID
    assert lib.rt_light_grid_host(None, 4, C.byref(info), None) == N.RT_E_INVALID
    assert lib.rt_light_grid_host(sc.desc_ptr, 4, None, None) == N.RT_E_INVALID
    # 27 lamps on a cubic lattice: 64^3 cells of 27 entries are more than 2^22, 53^3 are not (the largest that fit)
    from raytracer import scene as S
    b = rt.SceneBuilder()
    b.set_skybox(S.SkyBox.Nothing)
    for i in range(27):
        b.add(S.Sphere((float(i % 3), float(i // 3 % 3), float(i // 9)), 0.25),
              S.DiffuseLight(S.TextureLoader.solid(1.0, 1.0, 1.0)))
    cube = b.finalize(SEED)
    for cells, code in ((64, N.RT_E_INVALID), (54, N.RT_E_INVALID), (53, 0), (8, 0)):
        assert (code != 0) == (cells ** 3 * 27 > 1 << 22)
        if code or cells == 8:  # (the restatement of 53^3 rows is not worth its seconds)
            ref = G.grid_of(cube.desc, cells)
            assert ref.n == [cells] * 3 and ref.too_large == (code != 0)
        assert lib.rt_light_grid_host(cube.desc_ptr, cells, C.byref(info), None) == code, cells
        assert code or list(info.n) == [cells] * 3


def test_usage_names_the_flag():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--light-grid N" in r.stderr


@pytest.mark.parametrize("extra", [[], ["--ao", "1"], ["--denoise"]])
def test_light_grid_without_nee_or_direct_is_a_usage_error(extra):
    r = subprocess.run([CLI, "render", "cornell", "-w", "64", "-s", "4", "--light-grid", "4"] + extra,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "error: --light-grid" in r.stderr and "usage: ray-cli" in r.stderr and "rt_create" not in r.stderr


@pytest.mark.parametrize("mode", ["--nee", "--direct"])
def test_a_bad_light_grid_value_is_a_usage_error(mode):
    for v in ("-1", "65"):
        r = subprocess.run([CLI, "render", "cornell", "-w", "64", "-s", "4", mode, "--light-grid", v],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--light-grid N in 0 ... 64" in r.stderr
    r = subprocess.run([CLI, "render", "cornell", "-w", "64", "-s", "4", mode, "--light-grid"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "missing value for --light-grid" in r.stderr
