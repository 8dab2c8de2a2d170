"""Solid-angle sampling of rect lights on the CPU (rt_scene_light_sampling's third mode, added within ABI 11;
include/shirley_rt.h): rt_light_sample_host against the restatement of the header's text
(tests/rect_ref.py) bit for bit on a vertex set that holds the definition's edges, the third mode against the second
on sphere lights, the area and solid-angle estimators' agreement in expectation on the Cornell lamp, and the
interface (refusals, the header's text, ray-cli's --light-solid-angle).  Nothing here needs a GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import direct_ref as D
import lightgrid_ref as G
import raytracer as rt
import rect_ref as R
from raytracer import _native as N
from raytracer import scene as S
from test_light_cone import CLI, mismatches

SEED = 0x5EED
AREA, CONE, ALL = R.AREA, R.CONE, R.ALL
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case():
    """(scene, lights, points, normals, tags) of the hand-built scene (one rect light of each orientation, both
    emitter kinds): built once, shared, left unchanged."""
    sc = D.hand_scene(extras=True).finalize(SEED)
    lights, _ = D.list_lights(sc.desc)
    pts, nrm, tags = R.vertex_set(lights, SEED)
    return sc, lights, pts, nrm, tags


# ---- records ----------------------------------------------------------------------------------------
def test_the_vertex_set_holds_the_edges(case):
    """What the parity tests rely on: under the uniform pick every edge vertex samples the rect it was built for,
    every entry of EDGES occurs for every orientation, and the restatement sees the case each edge stands for."""
    _, lights, pts, nrm, tags = case
    assert len(pts) == 2000 and set(tags) == set(R.EDGES) | {None}
    seen, geoms = {}, {}
    for i, tag in enumerate(tags):
        if tag is None:
            continue
        x, n = list(pts[i]), list(nrm[i])
        rec = R.record(None, lights, ALL, SEED, i, x, n)
        _, geom, _, p, area, _ = lights[rec[0]]
        assert geom in D.RECTS, (i, tag)
        d1, d2, axis = D.RECTS[geom]
        e = max(p[1] - p[0], p[3] - p[2])
        v = R.rect_view(geom, p, x)
        geoms.setdefault(tag, set()).add(geom)
        seen.setdefault(tag, set()).add(rec[1])
        if tag == "coplanar":
            assert v.z0 == 0.0 and v.S is None and rec[1] == R.COPLANAR and rec[2] == 1 and rec[3:] == (0.0,) * 7
            continue
        assert rec[2] == 3, (i, tag)  # the pick's draw, then two exactly
        assert v.z0 < 0.0 and v.flip == (tag != "z-"), (i, tag)
        assert abs(v.S - R.solid_angle_atan(geom, p, x)) <= 1e-9 * v.S, (i, tag, v.S)
        if tag in ("z+", "z-"):
            assert v.z0 == -1.0 and rec[1] == 0 and rec[3 + axis] == (1.0 if tag == "z+" else -1.0), (i, tag)
        if tag == "corner":
            assert v.x0 == 0.0 and v.y0 == 0.0 and rec[1] == 0, (i, tag)
            assert rec[3 + d1] >= 0.0 and rec[3 + d2] >= 0.0
        if tag == "centre":
            assert v.x0 == -v.x1 and v.y0 == -v.y1 and rec[1] == 0, (i, tag)
        if tag in ("near10", "near40"):
            want = e * 2.0 ** (-10 if tag == "near10" else -40)
            assert abs(-v.z0 - want) <= 1e-3 * want and rec[1] == 0, (i, tag, v.z0)
            assert v.S > 6.0 and v.x0 <= rec[3 + d1] <= v.x1, (i, tag)  # nearly the whole hemisphere
        if tag == "horizon":  # cx = w[d1] / dist: the samples on the far half of the rect are cut
            assert (rec[1] == R.CUT) == (not rec[3 + d1] > 0.0), (i, tag)
        if tag in ("S+", "S-"):
            assert abs(v.S / R.MIN_S - (1.01 if tag == "S+" else 0.99)) < 1e-3, (i, tag, v.S)
            assert rec[1] == (0 if tag == "S+" else R.SMALL), (i, tag)
            if tag == "S-":  # the area form's record, but for the flag
                area_rec = R.record(None, lights, AREA, SEED, i, x, n)
                assert rec[:1] + rec[2:] == area_rec[:1] + area_rec[2:] and rec[8] > 0.0, (i, tag)
    assert all(len(g) == 3 for g in geoms.values()), geoms  # every orientation
    assert seen["horizon"] == {0, R.CUT}


@pytest.mark.parametrize("cells", [0, 3])
def test_host_records_equal_the_restatement(case, cells):
    sc, lights, pts, nrm, _ = case
    grid = G.Grid(lights, cells) if cells else None
    want = [R.record(grid, lights, ALL, SEED, i, list(pts[i]), list(nrm[i])) for i in range(len(pts))]
    got = rt.light_sample_host(sc, cells, ALL, pts, nrm, SEED)
    bad = mismatches(got, want)
    assert not bad, f"{len(bad)} fields differ, first {bad[:3]}"
    flags = [w[1] for w in want]
    assert flags.count(0) > 100 and flags.count(R.CUT) > 100 and flags.count(R.COPLANAR) > 10
    assert sum(1 for f in flags if f & R.SMALL) > 10
    assert {w[0] for w in want} == set(range(len(lights)))
    rect = [w for w in want if lights[w[0]][1] != N.RT_GEOM_SPHERE]
    assert all(w[2] == (1 if w[1] == R.COPLANAR else 3) for w in rect)
    assert all(w[8] == 0.0 and w[9] == 0.0 for w in rect if w[1] & R.ZERO)
    assert all(w[8] > 0.0 and 0.0 < w[9] < 1.0 for w in rect if not w[1] & R.ZERO)


def test_the_portable_trig_is_close_to_libm():
    """The restated pl_sin / pl_cos / pl_acos (the bits are checked through the records above) are the functions
    they are named after: within 4e-16 absolute of libm's over the arguments the sampler uses."""
    rs = np.random.RandomState(7)
    for a in list(rs.uniform(0.0, 2.0 * math.pi, 2000)) + [0.0, math.pi / 2, math.pi, 3 * math.pi / 2, 2 * math.pi]:
        assert abs(R.pl_sin(a) - math.sin(a)) <= 4e-16 and abs(R.pl_cos(a) - math.cos(a)) <= 4e-16, a
    for x in list(rs.uniform(-1.0, 1.0, 2000)) + [-1.0, -0.0, 0.0, 1.0]:
        assert abs(R.pl_acos(x) - math.acos(x)) <= 9e-16, x
    assert R.pl_acos(1.5) != R.pl_acos(1.5) and R.pl_sin(float("inf")) != R.pl_sin(float("inf"))


def test_mode_three_against_mode_one(case):
    """Sphere lights have the same record in modes 1 and 3, byte for byte, and the pick does not depend on the mode;
    rect lights differ."""
    sc, lights, pts, nrm, _ = case
    field = G.lamp_field().finalize(SEED)
    for scene, ls in ((sc, lights), (field, D.list_lights(field.desc)[0])):
        for cells in (0, 3):
            cone = rt.light_sample_host(scene, cells, CONE, pts, nrm, SEED)
            both = rt.light_sample_host(scene, cells, ALL, pts, nrm, SEED)
            assert [r.light for r in cone] == [r.light for r in both]
            sph = [i for i, r in enumerate(cone) if ls[r.light][1] == N.RT_GEOM_SPHERE]
            assert len(sph) > 300 and all(bytes(cone[i]) == bytes(both[i]) for i in sph)
            differ = sum(bytes(a) != bytes(b) for a, b in zip(cone, both))
            assert (differ > 300) == (scene is sc), differ  # (the lamp field holds no rect)


# ---- expectation ------------------------------------------------------------------------------------
LAMP = (213.0, 343.0, 227.0, 332.0, 554.0)  # the Cornell lamp: xz_rect x0, x1, z0, z1 at y
VERTICES = [  # (name, position, normal): the six vertices of the numpy check that came with the proposal
    ("floor under the lamp", (278.0, 0.0, 279.5), (0.0, 1.0, 0.0)),
    ("ceiling 5 beside", (348.0, 555.0, 280.0), (0.0, -1.0, 0.0)),
    ("ceiling 40 beside", (383.0, 555.0, 280.0), (0.0, -1.0, 0.0)),
    ("wall at mid height", (0.0, 277.0, 280.0), (1.0, 0.0, 0.0)),
    ("wall under the ceiling", (0.0, 540.0, 280.0), (1.0, 0.0, 0.0)),
    ("5000 below", (278.0, -4446.0, 279.5), (0.0, 1.0, 0.0)),
]


def test_both_modes_have_one_expectation_and_the_solid_angle_the_smaller_error():
    """One unoccluded DiffuseLight rect of the Cornell lamp's shape (so L = 1 and g_plain is the whole estimate),
    six vertices, 2^16 seeds each: the two modes' means of g_plain agree within 5 combined standard errors; the
    solid-angle form's standard error is below 0.6 of the area form's everywhere (1.4 x the worst figure of the
    proposal's numpy check, 0.42) and below 0.2 at the ceiling-5 vertex (numpy: 0.047; the area side's own error is
    heavy-tailed there), whose largest single estimate is below a tenth of the area form's.
    SE ratios, numpy check (libm trig, other draws) / this library (the restatement's bits, see above):
      floor under the lamp 0.25 / 0.250;  ceiling 5 beside 0.047 / 0.045 (largest estimate 0.022 against 6.13 /
      0.0222 against 6.059);  ceiling 40 beside 0.17 / 0.167;  wall at mid height 0.42 / 0.540;  wall under the
      ceiling 0.016 / 0.016;  5000 below 0.25 / 0.250.
    Means, area then solid angle: 0.0139459 +- 5.29e-07, 0.0139456 +- 1.32e-07;  0.00982929 +- 0.000473,
      0.0096384 +- 2.12e-05;  0.000113152 +- 7.98e-07, 0.00011213 +- 1.34e-07;  0.0139278 +- 7.08e-06,
      0.0139281 +- 3.83e-06;  0.00306056 +- 4.87e-06, 0.00306446 +- 7.92e-08;  0.000173765 +- 8.17e-11,
      0.000173765 +- 2.04e-11."""
    b = rt.SceneBuilder()
    b.set_skybox(S.SkyBox.Nothing)
    b.add(S.xz_rect(*LAMP), S.DiffuseLight(S.TextureLoader.solid(1.0, 1.0, 1.0)))
    sc = b.finalize(SEED)
    pts = np.array([v[1] for v in VERTICES])
    nrm = np.array([v[2] for v in VERTICES])
    n = 1 << 16
    g = {mode: np.array([[r.g_plain for r in rt.light_sample_host(sc, 0, mode, pts, nrm, seed)] for seed in range(n)])
         for mode in (AREA, ALL)}
    ratios, largest = [], {}
    for v, (name, _, _) in enumerate(VERTICES):
        m = {mode: float(g[mode][:, v].mean()) for mode in g}
        se = {mode: float(g[mode][:, v].std(ddof=1) / math.sqrt(n)) for mode in g}
        largest[v] = {mode: float(g[mode][:, v].max()) for mode in g}
        print(f"{name}: area {m[AREA]:.6g} +- {se[AREA]:.3g} (largest {largest[v][AREA]:.4g}), solid angle "
              f"{m[ALL]:.6g} +- {se[ALL]:.3g} (largest {largest[v][ALL]:.4g}), ratio {se[ALL] / se[AREA]:.3f}")
        assert m[ALL] > 0.0 and se[AREA] > 0.0
        assert abs(m[AREA] - m[ALL]) <= 5.0 * math.sqrt(se[AREA] ** 2 + se[ALL] ** 2), name
        ratios.append(se[ALL] / se[AREA])
    assert max(ratios) < 0.6, ratios
    assert ratios[1] < 0.2, ratios
    assert largest[1][ALL] < 0.1 * largest[1][AREA], largest[1]


# ---- interface --------------------------------------------------------------------------------------
def test_the_header_and_the_bindings_name_the_mode():
    with open(os.path.join(REPO, "include", "shirley_rt.h")) as f:
        text = f.read()
    assert "#define RT_ABI_VERSION 11" in text
    assert "enum { RT_LIGHT_SAMPLE_AREA = 0, RT_LIGHT_SAMPLE_SOLID_ANGLE = 1 };" in text
    assert "enum { RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL = 3 };" in text
    assert N.RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL == 3 and C.sizeof(N.rt_light_sample) == 72
    lib = N.rt_lib()
    for sym in ("rt_scene_light_sampling", "rt_light_sample_at", "rt_light_sample_host"):
        assert getattr(lib, sym) is not None


def test_invalid_arguments():
    lib = N.rt_lib()
    sc = D.hand_scene().finalize(SEED)
    p = np.zeros((1, 3))
    out = (N.rt_light_sample * 1)()
    pd = p.ctypes.data
    call = lambda cells, mode: lib.rt_light_sample_host(sc.desc_ptr, cells, mode, 1, pd, pd, SEED, out)  # noqa: E731
    assert call(0, ALL) == 0 and call(3, ALL) == 0
    for mode in (2, 4, -1):  # "rects only" is not offered
        assert call(0, mode) == N.RT_E_INVALID, mode
    assert call(65, ALL) == N.RT_E_INVALID
    assert lib.rt_light_sample_host(sc.desc_ptr, 0, ALL, 0, None, None, SEED, None) == 0
    assert lib.rt_light_sample_host(sc.desc_ptr, 0, ALL, 1, None, pd, SEED, out) == N.RT_E_INVALID
    with pytest.raises(rt.RtError) as e:
        rt.light_sample_host(sc, 0, 2, p, p, SEED)
    assert e.value.code == N.RT_E_INVALID


def test_usage_names_both_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--light-solid-angle" in r.stderr and "--light-cone" in r.stderr


@pytest.mark.parametrize("extra", [[], ["--light-cone"], ["--ao", "1"], ["--denoise"]])
def test_light_solid_angle_without_nee_or_direct_is_a_usage_error(extra):
    """Refused with the usage text before a device is opened (no rt_create message, whatever the machine has)."""
    r = subprocess.run([CLI, "render", "cornell", "-w", "64", "-s", "4", "--light-solid-angle"] + extra,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "error: --light-" in r.stderr and "usage: ray-cli" in r.stderr and "rt_create" not in r.stderr
