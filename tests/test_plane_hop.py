"""The plane-stack hop decision on the CPU (rt_device.h plane_hop_t, scene_compile.cpp plane_stack,
ScenePlacement.hop_planes).

tests/plane_hop_check.c restates the fast decision — the next plane of the sorted list in the ray's direction of
travel, at the correctly rounded quotient, answered only with origin and hit point inside the shrunk core — and the
host's plane_stack from the oracle's own functions, and compares every answered ray with the general decision
(tests/down_hop_check.c's), with the exhaustive closest hit under both test orders and with the reference's own walk;
tools/ground_stack prints the placement's word and the record itself."""
import json
import os
import subprocess

import pytest

import hop_scenes as HS
import raytracer as rt
from test_ground_hop import HOST, PKG, REPO, RT

SEED = 0x5EED
SEEDS = (SEED, 1, 7)
DRAWS = 300_000  # per stack

# the ground stacks of tests/hop_scenes.py that are plane stacks, and those that miss a premise: small_coat's core (its
# coat's extent) and rect_top's (its raised rect's) do not contain the guard rectangle; the tied stacks hold two
# planes closer than `gap`
PLANE = ["slab0", "slab_up", "slab_down", "floating", "bare", "neg_radius", "two_coats"]
NOT_PLANE = ["small_coat", "rect_top"] + HS.TIED
N_PLANES = {"two_coats": 6}  # (3 elsewhere: the rect, the coat's two faces)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plane_hop_check") / "plane_hop_check")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-w", "-o", exe, os.path.join(REPO, "tests", "plane_hop_check.c"),
                    "-lm", "-lpthread"], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def checks(checker, tmp_path_factory):
    """plane_hop_check's counts on random_scene's primitives for three seeds (with the coverage family) and on every
    kind-2 stack of tests/hop_scenes.py, all at once (a second or two each)."""
    tmp = tmp_path_factory.mktemp("plane_checks")
    procs = {}
    for seed in SEEDS:
        path = str(tmp / f"random_{seed}.prims")
        HS.write_prims(rt.scenes.random_scene(seed).finalize(seed), path)
        procs[f"random:{seed}"] = subprocess.Popen([checker, path, str(DRAWS), str(seed), "coverage"], stdout=subprocess.PIPE,
                                                   stderr=subprocess.PIPE, text=True)
    for name in HS.KIND2:
        path = str(tmp / (name + ".prims"))
        HS.write_prims(HS.scene(name), path)
        procs[name] = subprocess.Popen([checker, path, str(DRAWS), "7"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                       text=True)
    res = {}
    for name, p in procs.items():
        out, err = p.communicate(timeout=600)
        print(f"{name}: rc {p.returncode} {out.strip()} {err.strip()}")
        res[name] = (p.returncode, json.loads(out))
    return res


@pytest.mark.parametrize("name", [f"random:{s}" for s in SEEDS] + PLANE)
def test_no_answered_ray_differs(checks, name):
    """300 000 adversarial draws per stack — origins ulps either side of each plane, origins and hit points on, ulps
    off and mx either side of the core's edge, t around t_min and 2 t_min, slopes at the bound, exits at guarded
    cells: every ray the fast decision answers carries the general decision's (t bits, primitive, face, kind), the
    exhaustive closest hit's under both test orders and the reference's own walk's.  The draws do reach served and
    found answers, and answers among the fast path's own edge draws.  The controls (answers that would differ with
    mx = 0, answers that change with the standing-plane rule off) are printed by the fixture, not asserted."""
    rc, r = checks[name]
    assert r["ground_stack"] == 1 and r["plane_stack"] == 1 and r["draws"] == DRAWS
    assert r["planes"] == N_PLANES.get(name, 3)
    assert r["wrong"] == 0 and r["not_general"] == 0 and r["coverage_wrong"] == 0 and rc == 0
    assert r["served"] > DRAWS // 40 and r["found"] > DRAWS // 100 and r["edge_answers"] > DRAWS // 100


@pytest.mark.parametrize("name", NOT_PLANE)
def test_a_stack_that_misses_a_premise_is_no_plane_stack(checks, name):
    rc, r = checks[name]
    assert (rc, r["ground_stack"], r["plane_stack"]) == (3, 1, 0)


@pytest.mark.parametrize("seed", SEEDS)
def test_fast_decision_covers_the_general_one(checks, seed):
    """The cap on declines.  On a non-adversarial family on random_scene's stack — origins are the hit points of
    uniformly drawn rays, directions come from the refraction and Lambertian expressions — the fast decision
    declines at most 1 % of the rays the general decision answers: the margins are ~1e-12 of a ground 60 wide, so a
    higher rate would mean a wrong margin.  (Measured: 0 of ~95 000.)"""
    rc, r = checks[f"random:{seed}"]
    print(r["coverage_rays"], r["coverage_general"], r["coverage_declined"])
    assert r["coverage_rays"] == DRAWS // 3 and r["coverage_general"] > DRAWS // 6
    assert r["coverage_declined"] * 100 <= r["coverage_general"] and rc == 0


@pytest.fixture(scope="module")
def placements(tmp_path_factory):
    """tools/ground_stack on random_scene and every scene of tests/hop_scenes.py, under no variable and under
    SHIRLEY_HOP=general and SHIRLEY_HOP=up."""
    tmp = tmp_path_factory.mktemp("plane_placements")
    exe = str(tmp / "ground_stack")
    flags = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter"]
    srcs = [os.path.join(REPO, "tools", "ground_stack.cpp"), os.path.join(RT, "scene_compile.cpp"),
            os.path.join(RT, "bvh_build.cpp")] + [os.path.join(HOST, f) for f in ("scene.cpp", "scenes.cpp", "host_api.cpp",
                                                                                 "earth_embed.S")]
    subprocess.run(["g++"] + flags + ["-Wa,-I," + os.path.join(PKG, "assets"), "-o", exe] + srcs + ["-lz", "-ldl"], check=True,
                   timeout=900)
    cases = ["random", "random/HOP=general", "random/HOP=up"]
    for name in HS.NAMES:
        path = str(tmp / (name + ".json"))
        with open(path, "w") as f:
            f.write(HS.scene_json(name))
        cases += ["@" + path, "@" + path + "/HOP=general", "@" + path + "/HOP=up"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("SHIRLEY_")}
    out = subprocess.run([exe] + cases, check=True, capture_output=True, text=True, env=env, timeout=300).stdout
    res = {}
    for case, line in zip(cases, out.splitlines()):
        d = json.loads(line)
        name, _, keys = case.partition("/HOP=")
        res[os.path.splitext(os.path.basename(name))[0] if name.startswith("@") else name, keys or "default"] = d
        print(case, d)
    assert len(res) == len(cases) and all(r["status"] == 0 for r in res.values())
    return res


@pytest.mark.parametrize("name", ["random"] + HS.NAMES)
def test_hop_planes_follows_the_stack(placements, name):
    """hop_planes is set exactly for the plane stacks, never under SHIRLEY_HOP=general or =up; the instance is 4 there,
    and elsewhere what it was (3 for a ground stack with the down pass, 2 without, 1 without a ground stack);
    hop_kind stays what it was under all three."""
    kind = 2 if name == "random" else HS.KIND[name]
    plane = name == "random" or name in PLANE
    for mode in ("default", "general", "up"):
        r = placements[name, mode]
        assert (r["hop_pass"], r["hop_kind"], r["stats_hop_kind"]) == (1, kind, kind), mode
        assert r["hop_planes"] == (1 if plane and mode == "default" else 0), mode
        want = 1 if kind == 1 else (2 if mode == "up" else (4 if plane and mode == "default" else 3))
        assert r["hop_instance"] == want, mode


@pytest.mark.parametrize("name", ["random"] + PLANE)
def test_plane_record_is_the_restated_one(placements, checks, name):
    """The record scene compilation uploads — the sorted planes, each one's face, answer and top-plane bit, the shrunk
    core and tol — is, bit for bit, the one tests/plane_hop_check.c restates and checks."""
    r = placements[name, "default"]
    c = checks[f"random:{SEED}" if name == "random" else name][1]
    assert r["planes"] == c["plane_y"] and [i & 31 for i in r["plane_info"]] == c["plane_code"]
    assert r["core"] == c["core"] and r["tol"] == c["tol_hex"]
