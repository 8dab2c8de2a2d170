"""The traversal's closed-form answer about a plane stack on the CPU (rt_device.h plane_first,
scene_compile.cpp plane_stack, rt_layout.h DPlanes).

tests/ground_first_check.c restates plane_first — "none", or the first plane ahead of the origin and beyond tol at
the correctly rounded quotient, answered only under the widened premises — and the host's record from the oracle's
own functions, and compares every answer with what the leaves of G return by the reference's rule, G walked in
either order; tools/ground_stack prints the record scene compilation uploads."""
import json
import os
import subprocess

import pytest

import ground_first_scenes as GS
import hop_scenes as HS
import raytracer as rt
from test_ground_hop import HOST, PKG, REPO, RT
from test_plane_hop import NOT_PLANE, PLANE

SEED = 0x5EED
SEEDS = (SEED, 1, 7)
DRAWS = 300_000  # per stack


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ground_first_check") / "ground_first_check")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-w", "-o", exe, os.path.join(REPO, "tests", "ground_first_check.c"),
                    "-lm", "-lpthread"], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def checks(checker, tmp_path_factory):
    """ground_first_check's counts on random_scene's primitives for three seeds (with the coverage family) and on
    every kind-2 stack of tests/hop_scenes.py, all at once (a second or two each)."""
    tmp = tmp_path_factory.mktemp("first_checks")
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
def test_no_answer_differs(checks, name):
    """300 000 adversarial draws per stack — origins ulps either side of each plane, of Y + tol and of Y + H, origins
    and hit points on, ulps off and a margin either side of the core's and the grown extent's edges, t around t_min
    and 2 t_min, slopes at the bound, upward rays from tol above Y: every "hit" carries the (t bits, primitive, face)
    that G's leaves return under both walk orders, and after every "none" they return nothing.  The draws do reach
    hits from inside the stack and from above it, both kinds of "none", and answers among the edge draws.  The
    controls (answers given only with mx = mo = 0, with tol = 0, without the H bound) are printed by the fixture, not
    asserted."""
    rc, r = checks[name]
    assert r["ground_stack"] == 1 and r["plane_stack"] == 1 and r["draws"] == DRAWS
    assert r["wrong"] == 0 and r["coverage_wrong"] == 0 and rc in (0, 4)
    assert r["hits"] > DRAWS // 20 and r["hits_from_above"] > DRAWS // 100 and r["edge_answers"] > DRAWS // 100
    assert r["nones_upward"] > DRAWS // 100 and r["nones_over_edge"] > DRAWS // 1000


@pytest.mark.parametrize("name", NOT_PLANE)
def test_a_stack_that_misses_a_premise_is_no_plane_stack(checks, name):
    rc, r = checks[name]
    assert (rc, r["ground_stack"], r["plane_stack"]) == (3, 1, 0)


@pytest.mark.parametrize("seed", SEEDS)
def test_plane_first_covers_what_a_render_traces(checks, seed):
    """The cap on declines, carried over from tests/test_plane_hop.py: of the family a render produces on
    random_scene — camera rays of the headline camera, and rays from the hit points of uniformly drawn rays with
    refraction, reflection and Lambertian directions — plane_first declines at most 1 %; above it too many waves run
    the fallback loops for one lane."""
    rc, r = checks[f"random:{seed}"]
    print(r["coverage_rays"], r["coverage_camera"], r["coverage_declined"], r["coverage_camera_declined"], r["coverage_none"])
    assert r["coverage_rays"] == DRAWS // 3 and r["coverage_camera"] >= DRAWS // 9
    assert r["coverage_declined"] * 100 <= r["coverage_rays"] and rc == 0


@pytest.fixture(scope="module")
def placements(tmp_path_factory):
    """tools/ground_stack (the host's scene compilation, no HIP) on random_scene, every plane stack of
    tests/hop_scenes.py and tests/ground_first_scenes.py's own, under a default upload."""
    tmp = tmp_path_factory.mktemp("first_placements")
    exe = str(tmp / "ground_stack")
    flags = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter"]
    srcs = [os.path.join(REPO, "tools", "ground_stack.cpp"), os.path.join(RT, "scene_compile.cpp"),
            os.path.join(RT, "bvh_build.cpp")] + [os.path.join(HOST, f) for f in ("scene.cpp", "scenes.cpp", "host_api.cpp",
                                                                                 "earth_embed.S")]
    subprocess.run(["g++"] + flags + ["-Wa,-I," + os.path.join(PKG, "assets"), "-o", exe] + srcs + ["-lz", "-ldl"], check=True,
                   timeout=900)
    names = PLANE + GS.NAMES
    cases = ["random"]
    for name in names:
        path = str(tmp / (name + ".json"))
        with open(path, "w") as f:
            f.write(GS.scene_json(name))
        cases.append("@" + path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SHIRLEY_")}
    out = subprocess.run([exe] + cases, check=True, capture_output=True, text=True, env=env, timeout=300).stdout
    res = {name: json.loads(line) for name, line in zip(["random"] + names, out.splitlines())}
    for name, d in res.items():
        print(name, d)
    assert len(res) == len(cases) and all(r["status"] == 0 and r["hop_instance"] == 4 for r in res.values())
    return res


@pytest.mark.parametrize("name", ["random"] + PLANE)
def test_first_record_is_the_restated_one(placements, checks, name):
    """The part of the record plane_first reads — its own core, the grown extent and Y + H — is, bit for bit, the one
    tests/ground_first_check.c restates and checks."""
    r = placements[name]
    c = checks[f"random:{SEED}" if name == "random" else name][1]
    assert r["planes"] == c["plane_y"]
    assert r["core_first"] == c["core_first"] and r["outer"] == c["outer"] and r["y_max"] == c["y_max"]


def test_a_large_sphere_is_a_leaf_of_the_root(placements):
    """tests/test_gpu_ground_first.py's `big_ball` stack: its large sphere is a direct leaf child of the first node a
    traversal visits, beside the stack's own leaves, so a lane that skips those still tests it there."""
    r = placements["big_ball"]
    assert 0 in r["root_leaf_kinds"] and any(k != 0 for k in r["root_leaf_kinds"]), r
