"""Scene compilation on the CPU (csrc/rt/scene_compile.cpp through tools/scene_plan): the digest, the
placement plan (which kernel instance every frame runs: wide or narrow block; nodes, primitives, Perlin and
material tables in LDS; optimal or greedy collapse), the tree's sizes and an FNV-1a of every compiled device
table, for every builtin scene with both builders, the placement flags and the upload-time tuning switches.
Compared with tests/golden/scene_plan.json, which was recorded from the commit before scene compilation
left rt_api.cpp (its `provenance` says how), so the plan and the tables are pinned to what rt_scene_upload
computed then."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "shirley-raytracing-rs_amd")
RT = os.path.join(PKG, "csrc", "rt")
HOST = os.path.join(PKG, "csrc", "host")
GOLDEN = os.path.join(REPO, "tests", "golden", "scene_plan.json")
SEED = "0x5EED"
BUILTINS = ["random", "random-night", "demo", "perlin", "earth", "box-light", "cornell", "final", "final:4:30",
            "final:6:60", "spheres:11"]


def case(scene, builder="sah", placement="default", tuning=""):
    return f"{scene}/{SEED}/{builder}/{placement}" + (f"/{tuning}" if tuning else "")


SCENES = [case(s, b) for s in BUILTINS + ["empty", "one"] for b in ("reference", "sah")]
PLACEMENT_FLAGS = [case(s, b, p)
                   for s, b in (("random", "sah"), ("cornell", "reference"), ("final:4:30", "sah"),
                                ("spheres:11", "sah"), ("spheres:11", "reference"))
                   for p in ("global", "half_lds", "lds")]
TUNING = [case("final", tuning="NO_WIDE=1"), case("final:4:30", tuning="NO_WIDE=1"),
          case("random", tuning="NO_LDS_MATS=1"), case("random", tuning="NO_LDS_PRIMS=1"),
          case("random", tuning="NO_LDS_PERLIN=1"), case("perlin", tuning="NO_LDS_PERLIN=1"),
          case("random", tuning="WF_EXTEND2=1"), case("random", tuning="SAH_BINNED=1"),
          case("cornell", tuning="SAH_BOXW=1"), case("cornell", "reference", tuning="SPLIT_NT=4,SPLIT_REFILL=3")]
TUNING += [case(s, b, tuning=f"COLLAPSE_DP={v}") for s in ("cornell", "spheres:11") for b in ("reference", "sah")
           for v in (0, 1)]
TUNING += [case("spheres:11", tuning="LDS_NODES=100"), case("spheres:11", tuning="LDS_NODES=1000000"),
           case("spheres:11", "sah", "lds", "LDS_NODES=100")]
# gen_spheres on either side of each decision flip (the fixture's provenance names the sweep): primitives
# beside the wide block's tree and the optimal collapse up to side 3, the wide block up to side 4 / 5
FLIPS = [case(f"spheres:{k}", b) for k in (3, 4, 5, 6) for b in ("reference", "sah")]
CASES = SCENES + PLACEMENT_FLAGS + TUNING + FLIPS


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """Every case's line of tools/scene_plan, built here with g++ alone (no HIP include path) and run once."""
    exe = str(tmp_path_factory.mktemp("scene_plan") / "scene_plan")
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror"]
    objs = []
    for src in (os.path.join(REPO, "tools", "scene_plan.cpp"), os.path.join(RT, "scene_compile.cpp")):
        objs.append(exe + "_" + os.path.basename(src) + ".o")
        subprocess.run(["g++"] + flags + ["-c", src, "-o", objs[-1]], check=True, timeout=300)
    host = [os.path.join(HOST, f) for f in ("scene.cpp", "scenes.cpp", "host_api.cpp", "earth_embed.S")]
    subprocess.run(["g++"] + flags + ["-Wno-unused-parameter", "-Wa,-I," + os.path.join(PKG, "assets"), "-o", exe] + objs +
                   [os.path.join(RT, "bvh_build.cpp")] + host + ["-lz", "-ldl"], check=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SHIRLEY_")}
    out = subprocess.run([exe] + CASES, check=True, capture_output=True, text=True, env=env, timeout=300).stdout
    res = {}
    for line in out.splitlines():
        d = json.loads(line)
        res[d.pop("case")] = d
    return res


def test_fixture_holds_exactly_these_cases(golden):
    assert len(set(CASES)) == len(CASES)
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_plan_and_tables_match_the_parent(plans, golden, name):
    got, want = plans[name], golden[name]
    assert got["status"] == 0 == want["status"]
    diff = {k: (got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)}
    assert not diff, f"{name}: (got, parent) {diff}"


def test_the_flips_are_flips(golden):
    # the fixture's own story: what the pairs of sides are there to pin
    for b in ("reference", "sah"):
        s = {k: golden[case(f"spheres:{k}", b)] for k in (3, 4, 5, 6)}
        assert (s[3]["n_lds_prims"], s[4]["n_lds_prims"]) == (s[3]["n_objects"], 0)
        assert (s[3]["collapse_dp"], s[4]["collapse_dp"]) == (1, 0)
        last_wide = 4 if b == "reference" else 5
        assert (s[last_wide]["wide"], s[last_wide + 1]["wide"]) == (1, 0)


def test_scene_compile_reads_the_environment_in_one_place():
    with open(os.path.join(RT, "scene_compile.cpp")) as f:
        src = f.read()
    body = src[src.index("SceneTuning tuning_from_env() {"):]
    body = body[:body.index("\n}\n")]
    assert src.count("getenv") == body.count("getenv") > 0
    assert "hip/" not in src
