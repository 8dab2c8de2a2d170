"""The ground-stack hop pass on the CPU (rt_device.h ground_hop, scene_compile.cpp ground_stack).

tests/ground_hop_check.c restates the pass's serve decision from the oracle's own functions and compares every
served ray with the exhaustive closest hit over all primitives, by the reference's rules, on random_scene's
primitives for three seeds; tools/ground_stack prints the kind of hop pass scene compilation chooses and checks the
guard bitmap it builds by brute force."""
import json
import os
import subprocess

import pytest

import raytracer as rt
from raytracer import _native as N

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "shirley-raytracing-rs_amd")
RT = os.path.join(PKG, "csrc", "rt")
HOST = os.path.join(PKG, "csrc", "host")
SEED = 0x5EED
SEEDS = (SEED, 1, 7)
DRAWS = 700_000  # per seed: 2.1 M rays in all


def write_prims(scene, path):
    """One line per primitive of a finalized scene: kind, dielectric, p0 .. p5 as hex floats."""
    d = scene.desc
    kinds = {N.RT_GEOM_SPHERE: 0, N.RT_GEOM_RECT_XZ: 3, N.RT_GEOM_RECT_BOX: 4}
    with open(path, "w") as f:
        for i in range(d.n_objects):
            o = d.objects[i]
            diel = int(d.materials[o.material].kind == N.RT_MAT_DIELECTRIC)
            f.write(" ".join([str(kinds[o.geometry]), str(diel)] + [float(o.p[k]).hex() for k in range(6)]) + "\n")


def test_no_served_ray_differs_from_the_exhaustive_closest_hit(tmp_path):
    """Zero served rays whose ground-only answer differs from the exhaustive one in primitive, face or t, over
    2.1 M adversarial draws; and the check bites: with the guard bitmap switched off some would differ (rays that
    leave the coat within ~5e-8 of a contact point, where the reference's sphere root wins or ties), and so would
    some with the slope bounds off.  Measured: served 67 892 of 300 000 draws, 7 440 wrong without the guard, 36
    without the slope bounds, largest flip distance 4.8e-8 (seed 0x5EED)."""
    exe = str(tmp_path / "ground_hop_check")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-w", "-o", exe, os.path.join(REPO, "tests", "ground_hop_check.c"),
                    "-lm", "-lpthread"], check=True, timeout=300)
    procs = []
    for seed in SEEDS:
        path = str(tmp_path / f"prims_{seed}.txt")
        write_prims(rt.scenes.random_scene(seed).finalize(seed), path)
        procs.append(subprocess.Popen([exe, path, str(DRAWS), str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True))
    total = {"served": 0, "wrong_without_guard": 0, "wrong_without_slope": 0}
    for seed, p in zip(SEEDS, procs):
        out, err = p.communicate(timeout=600)
        print(f"seed {seed:#x}: {out.strip()} {err.strip()}")
        r = json.loads(out)
        assert p.returncode == 0 and r["ground_stack"] == 1 and r["draws"] == DRAWS
        assert r["served_wrong"] == 0
        assert r["served"] > DRAWS // 10 and r["top_exits"] > DRAWS // 20  # the draws do reach the pass
        for k in total:
            total[k] += r[k]
    assert total["wrong_without_guard"] > 0 and total["wrong_without_slope"] > 0


def variant(edit):
    """random_scene's JSON with `edit` applied to its object list."""
    src = json.loads(rt.scenes.random_scene(SEED).to_json())
    src["objects"] = edit(src["objects"])
    return json.dumps(src)


def moved(objs, dy):
    """The first small sphere moved by dy along y."""
    out, done = [], False
    for o in objs:
        if not done and "Sphere" in o["geometry"] and o["geometry"]["Sphere"]["radius"] < 0.5:
            o = json.loads(json.dumps(o))
            o["geometry"]["Sphere"]["center"]["vec"][1] += dy
            done = True
        out.append(o)
    assert done
    return out


def doubled(objs):
    """tests/test_gpu_hop.py tied_scene_in_lds("dielectric"): every third sphere, the rect and the coat, twice."""
    red = {"Lambertian": {"albedo": {"Solid": {"vec": [0.9, 0.1, 0.05]}}}}
    out, n = [], 0
    for o in objs:
        if "Sphere" in o["geometry"]:
            n += 1
            if n % 3:
                continue
        out.append(o)
        out.append(o if "RectBox" in o["geometry"] else {**o, "material": red})
    return out


def spread(objs):
    """Two spheres moved 40 apart in x and z, still resting on the coat: a guard bitmap of 1 280 x 1 280 cells
    and more, beyond its 128 KiB."""
    out, k = [], 0
    for o in objs:
        if "Sphere" in o["geometry"] and o["geometry"]["Sphere"]["radius"] < 0.5 and k < 2:
            o = json.loads(json.dumps(o))
            c = o["geometry"]["Sphere"]["center"]["vec"]
            c[0] = c[2] = -20.0 if k == 0 else 20.0
            k += 1
        out.append(o)
    assert k == 2
    return out


FILES = {"lowered": lambda o: moved(o, -1e-3), "raised": lambda o: moved(o, 0.25), "doubled": doubled, "spread": spread}
BUILTIN = ["random", "random-night", "cornell", "earth", "random/HOP=root", "random/NO_HOP=1"]


@pytest.fixture(scope="module")
def modes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ground_stack")
    exe = str(tmp / "ground_stack")
    flags = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter"]
    srcs = [os.path.join(REPO, "tools", "ground_stack.cpp"), os.path.join(RT, "scene_compile.cpp"),
            os.path.join(RT, "bvh_build.cpp")] + [os.path.join(HOST, f) for f in ("scene.cpp", "scenes.cpp", "host_api.cpp",
                                                                                 "earth_embed.S")]
    subprocess.run(["g++"] + flags + ["-Wa,-I," + os.path.join(PKG, "assets"), "-o", exe] + srcs + ["-lz", "-ldl"], check=True,
                   timeout=900)
    cases = list(BUILTIN)
    for name, edit in FILES.items():
        path = str(tmp / (name + ".json"))
        with open(path, "w") as f:
            f.write(variant(edit))
        cases.append("@" + path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SHIRLEY_")}
    out = subprocess.run([exe] + cases, check=True, capture_output=True, text=True, env=env, timeout=300).stdout
    res = {}
    for line in out.splitlines():
        d = json.loads(line)
        name = d.pop("case")
        res[os.path.splitext(os.path.basename(name))[0] if name.startswith("@") else name] = d
        print(name, d)
    assert all(r["status"] == 0 and r["hop_kind"] == r["stats_hop_kind"] for r in res.values())
    return res


@pytest.mark.parametrize("case,kind", [("random", 2), ("random-night", 0), ("cornell", 0), ("earth", 0), ("lowered", 1),
                                       ("raised", 2), ("doubled", 2), ("spread", 1), ("random/HOP=root", 1),
                                       ("random/NO_HOP=1", 0)])
def test_the_mode_scene_compilation_chooses(modes, case, kind):
    r = modes[case]
    assert r["hop_kind"] == kind and r["hop_pass"] == (1 if kind else 0)
    if case == "doubled":
        assert (r["n"], r["n_box"]) == (4, 2)
    if case == "random":
        assert (r["n"], r["n_box"]) == (2, 1) and (r["y_top"], r["y_lo"] < -0.02 < -0.01 < r["y_hi"]) == (0.0, True)


@pytest.mark.parametrize("case", ["random", "raised", "doubled"])
def test_the_guard_bitmap_against_brute_force(modes, case):
    """Every cell marked exactly when its rectangle comes within the guard radius of some guarded contact point,
    over all spheres; 256 points on and inside every guard circle all fall in marked cells; within 128 KiB."""
    r = modes[case]
    assert r["cells_wrong"] == 0 and r["points_free"] == 0
    assert 0 < r["cells_marked"] < r["nx"] * r["nz"] // 20 and r["guard_bytes"] <= 128 * 1024
