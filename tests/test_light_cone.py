"""Solid-angle sampling of sphere lights on the CPU (include/shirley_rt.h, added within ABI 11):
rt_light_sample_host against the restatement of the header's text (tests/cone_ref.py) bit for bit on a vertex set
that holds the definition's edges, the two modes' agreement in expectation, rect lights, and ray-cli's
--light-cone.  Nothing here needs a GPU."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import cone_ref as K
import direct_ref as D
import lightgrid_ref as G
import nee_ref as R
import raytracer as rt
from raytracer import _native as N
from raytracer import scene as S

CLI = os.path.join(N.BIN_DIR, "ray-cli")
SEED = 0x5EED
AREA, CONE = K.AREA, K.CONE
FIELDS = ("light", "flags", "draws", "w0", "w1", "w2", "cx", "cy", "g_plain", "g_mis")


def bits(v):
    """A value's bits: -0.0 and +0.0 differ, every NaN is one value."""
    return "nan" if v != v else struct.pack("<d", float(v))


def unpack(r):
    return (r.light, r.flags, r.draws, r.w[0], r.w[1], r.w[2], r.cx, r.cy, r.g_plain, r.g_mis)


def mismatches(got, want):
    """[(vertex, field, got, want)] of the records that differ in any bit."""
    out = []
    for i, (g, w) in enumerate(zip(got, want)):
        g = unpack(g)
        out += [(i, f, a, b) for f, a, b in zip(FIELDS, g, w) if bits(a) != bits(b)]
    return out


SCENES = {"hand": lambda: D.hand_scene(extras=True).finalize(SEED), "lamps": lambda: G.lamp_field().finalize(SEED)}


@pytest.fixture(scope="module", params=sorted(SCENES))
def case(request):
    """(name, scene, lights, points, normals, tags): built once per scene, shared, left unchanged."""
    sc = SCENES[request.param]()
    lights, _ = D.list_lights(sc.desc)
    pts, nrm, tags = K.vertex_set(lights, SEED)
    return request.param, sc, lights, pts, nrm, tags


def test_library_exports_the_symbols_within_abi_11():
    lib = N.rt_lib()
    for sym in ("rt_scene_light_sampling", "rt_light_sample_at", "rt_light_sample_host"):
        assert sym in N.RT_SIGNATURES and getattr(lib, sym) is not None
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "shirley_rt.h")) as f:
        text = f.read()
    assert "#define RT_ABI_VERSION 11" in text
    assert "RT_LIGHT_SAMPLE_AREA = 0, RT_LIGHT_SAMPLE_SOLID_ANGLE = 1" in text
    assert (N.RT_LIGHT_SAMPLE_AREA, N.RT_LIGHT_SAMPLE_SOLID_ANGLE) == (0, 1)
    import ctypes as C
    assert C.sizeof(N.rt_light_sample) == 72


def test_the_vertex_set_holds_the_edges(case):
    """What the parity test below relies on: under the uniform pick every edge vertex samples the light it was
    built for, every entry of EDGES occurs, and the cone's restatement sees the cases the edges stand for."""
    name, _, lights, pts, nrm, tags = case
    assert len(pts) == 2000 and set(tags) == set(K.EDGES) | {None}
    seen = {}
    az = set()
    on_surface = 0
    for i, tag in enumerate(tags):
        if tag is None:
            continue
        rec = K.record(None, lights, CONE, SEED, i, list(pts[i]), list(nrm[i]))
        c, r = lights[rec[0]][3][0:3], lights[rec[0]][3][3]
        assert lights[rec[0]][1] == N.RT_GEOM_SPHERE
        wc, dc2, om = K.cone_of(c, r, list(pts[i]))
        want = {"near40": r * (1.0 + 2.0 ** -40), "near10": r * (1.0 + 2.0 ** -10), "far": 1e6 * r}.get(tag)
        if want is not None:  # (the vertex is the edge of the light it samples)
            assert abs(math.sqrt(dc2) - want) <= 1e-9 * want and om is not None, (i, tag)
        if tag in ("inside", "centre", "surface"):
            assert dc2 <= r * r * (1.0 + 1e-15), (i, tag)
            on_surface += tag == "surface" and dc2 == r * r
        if tag in ("inside", "centre"):
            assert rec[1] == K.INSIDE and rec[2] == 1 and rec[3:] == (0.0,) * 7, (i, tag)
        if tag.startswith("az"):
            a_z = wc[2] / math.sqrt(dc2)
            az.add(bits(a_z))
            assert bits(a_z) == bits({"az-1": -1.0, "az+1": 1.0, "az+0": 0.0,
                                      "az-0": -0.0 if c[2] == 0.0 else 0.0}[tag]), (i, tag)
        if tag == "away":
            assert rec[1] == K.CUT and rec[6] < 0.0, (i, tag)
        seen.setdefault(tag, set()).add(rec[1])
    assert on_surface > 0, "no vertex lies exactly on a sphere"
    assert {bits(-1.0), bits(1.0), bits(0.0)} <= az and ((bits(-0.0) in az) == (name == "lamps"))
    assert seen["near40"] == {0} and seen["near10"] == {0} and seen["far"] == {0}
    # the tangent plane at the cone's edge has the whole cone on one side: cx changes sign with the normal, and
    # is 0 up to rounding for a sample on the edge itself
    assert seen["tangent+"] | seen["tangent-"] == {0, K.CUT}


@pytest.mark.parametrize("cells", [0, 3])
@pytest.mark.parametrize("mode", [AREA, CONE])
def test_host_records_equal_the_restatement(case, cells, mode):
    _, sc, lights, pts, nrm, _ = case
    grid = G.Grid(lights, cells) if cells else None
    want = [K.record(grid, lights, mode, SEED, i, list(pts[i]), list(nrm[i])) for i in range(len(pts))]
    got = rt.light_sample_host(sc, cells, mode, pts, nrm, SEED)
    bad = mismatches(got, want)
    assert not bad, f"{len(bad)} fields differ, first {bad[:3]}"
    flags = [w[1] for w in want]
    assert flags.count(0) > 100 and flags.count(K.CUT) > 100 and (flags.count(K.INSIDE) > 0) == (mode == CONE)
    assert {w[0] for w in want} == set(range(len(lights)))
    if mode == CONE:  # two draws per disk attempt after the pick's one; no sample lands on the far side
        sph = [w for w in want if lights[w[0]][1] == N.RT_GEOM_SPHERE and w[1] != K.INSIDE]
        assert all(w[2] % 2 == 1 for w in sph) and any(w[2] > 3 for w in sph)
        assert all(w[7] > -1e-7 for w in sph), "a cone sample on the sphere's far side"


def test_area_mode_is_the_earlier_restatements():
    """cone_ref's light sample in mode AREA against nee_ref's (uniform pick) and lightgrid_ref's (grid pick)."""
    sc = D.hand_scene(extras=True).finalize(SEED)
    lights, _ = D.list_lights(sc.desc)
    pts, nrm, _ = K.vertex_set(lights, SEED, 200)
    grid = G.Grid(lights, 3)
    lit = lambda r6: False  # noqa: E731
    a = [0.5, 0.25, 0.125]
    for mis in (False, True):
        for i in range(len(pts)):
            x, n = list(pts[i]), list(nrm[i])
            v, d, _ = K.light_sample(None, lights, AREA, SEED, i, 0, 0, x, n, a, lit, mis)
            assert (v, d) == R.light_sample(lights, SEED, i, 0, 0, x, n, a, lit, mis)
            assert K.light_sample(grid, lights, AREA, SEED, i, 0, 0, x, n, a, lit, mis) == \
                G.light_sample(grid, lights, SEED, i, 0, 0, x, n, a, lit, mis)


def test_rect_lights_have_the_same_record_in_both_modes(case):
    name, sc, lights, pts, nrm, _ = case
    for cells in (0, 3):
        area = rt.light_sample_host(sc, cells, AREA, pts, nrm, SEED)
        cone = rt.light_sample_host(sc, cells, CONE, pts, nrm, SEED)
        rect = [i for i, r in enumerate(area) if lights[r.light][1] != N.RT_GEOM_SPHERE]
        assert (len(rect) > 300) == (name == "hand")
        assert all(bytes(area[i]) == bytes(cone[i]) for i in rect)
        assert [r.light for r in area] == [r.light for r in cone]  # (the pick does not depend on the mode)
        assert any(bytes(a) != bytes(c) for a, c in zip(area, cone))


# ---- expectation ------------------------------------------------------------------------------------
LAMP_C, LAMP_R = (0.0, 2.0, 0.0), 0.4
# the lamp's centre seen from the vertex (normal +y): the plain, the grazing and the nearly touching case of the
# numpy check that came with the proposal
OFFSETS = [(0.3, 1.5, -0.2), (2.0, 0.3, 1.0), (0.1, 0.45, 0.0)]


def test_both_modes_have_one_expectation_and_the_cone_the_smaller_error():
    """One unoccluded DiffuseLight sphere (so L = 1 and g_plain is the whole estimate of the vertex's irradiance
    over pi), three vertices, 2^16 seeds each: the two modes' means of g_plain agree within 5 combined standard
    errors, and the cone's standard error is below half the area's at every vertex (the bound the proposal's numpy
    check suggested: 0.02 - 0.33 there).  Measured (the library gives the restatement's bits, see above), area then
    cone: plain 0.065869 +- 0.000462, 0.065370 +- 0.0000085, ratio 0.018; grazing 0.0042523 +- 0.0000318,
    0.0042247 +- 0.0000106, ratio 0.333; nearly touching 0.76364 +- 0.0272, 0.73382 +- 0.00068, ratio 0.025."""
    b = rt.SceneBuilder()
    b.set_skybox(S.SkyBox.Nothing)
    b.add(S.Sphere(LAMP_C, LAMP_R), S.DiffuseLight(S.TextureLoader.solid(1.0, 1.0, 1.0)))
    sc = b.finalize(SEED)
    pts = np.array([[LAMP_C[a] - o[a] for a in range(3)] for o in OFFSETS])
    nrm = np.array([[0.0, 1.0, 0.0]] * 3)
    n = 1 << 16
    g = {mode: np.array([[r.g_plain for r in rt.light_sample_host(sc, 0, mode, pts, nrm, seed)] for seed in range(n)])
         for mode in (AREA, CONE)}
    ratios = []
    for v in range(3):
        m = {mode: float(g[mode][:, v].mean()) for mode in g}
        se = {mode: float(g[mode][:, v].std(ddof=1) / math.sqrt(n)) for mode in g}
        print(f"vertex {v}: area {m[AREA]:.6g} +- {se[AREA]:.3g}, cone {m[CONE]:.6g} +- {se[CONE]:.3g}, "
              f"ratio {se[CONE] / se[AREA]:.3f}")
        assert m[CONE] > 0.0 and se[AREA] > 0.0
        assert abs(m[AREA] - m[CONE]) <= 5.0 * math.sqrt(se[AREA] ** 2 + se[CONE] ** 2), v
        ratios.append(se[CONE] / se[AREA])
    assert max(ratios) < 0.5, ratios


# ---- refusals ---------------------------------------------------------------------------------------
def test_invalid_arguments():
    lib = N.rt_lib()
    sc = D.hand_scene().finalize(SEED)
    p = np.zeros((1, 3))
    out = (N.rt_light_sample * 1)()
    call = lambda d, cells, mode, n, a, b, o: lib.rt_light_sample_host(d, cells, mode, n, a, b, SEED, o)  # noqa: E731
    pd = p.ctypes.data
    assert call(sc.desc_ptr, 0, CONE, 1, pd, pd, out) == 0
    assert call(sc.desc_ptr, 0, CONE, 0, None, None, None) == 0
    for cells, mode in ((-1, AREA), (65, AREA), (0, -1), (0, 2)):
        assert call(sc.desc_ptr, cells, mode, 1, pd, pd, out) == N.RT_E_INVALID, (cells, mode)
    assert call(None, 0, AREA, 1, pd, pd, out) == N.RT_E_INVALID
    assert call(sc.desc_ptr, 0, AREA, -1, pd, pd, out) == N.RT_E_INVALID
    for args in ((None, pd, out), (pd, None, out), (pd, pd, None)):
        assert call(sc.desc_ptr, 0, AREA, 1, *args) == N.RT_E_INVALID
    dark = rt.scenes.random_scene(SEED).finalize(SEED)  # no listed light
    assert call(dark.desc_ptr, 0, CONE, 1, pd, pd, out) == N.RT_E_INVALID
    with pytest.raises(rt.RtError) as e:
        rt.light_sample_host(dark, 0, CONE, p, p, SEED)
    assert e.value.code == N.RT_E_INVALID


def test_usage_names_the_flag():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--light-cone" in r.stderr


@pytest.mark.parametrize("extra", [[], ["--ao", "1"], ["--denoise"]])
def test_light_cone_without_nee_or_direct_is_a_usage_error(extra):
    """Refused with the usage text before a device is opened (no rt_create message, whatever the machine has)."""
    r = subprocess.run([CLI, "render", "cornell", "-w", "64", "-s", "4", "--light-cone"] + extra,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "error: --light-cone" in r.stderr and "usage: ray-cli" in r.stderr and "rt_create" not in r.stderr
