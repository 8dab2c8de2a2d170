"""The down pass's decision on the CPU (rt_device.h ground_hop_t<true>, scene_compile.cpp
ScenePlacement.hop_down).

tests/down_hop_check.c restates the extended decision — served as before, or *found*: a non-dielectric hit of the
ground stack on a plane at least `gap` below its top — from the oracle's own functions and compares every served and
found ray with the exhaustive closest hit (the stack tested first and last) and with the reference's own walk of its
own tree, which alone judges the stacks with exact ties; tools/ground_stack prints hop_down, the placement's word
on whether a stack has such a member at all."""
import json
import os
import subprocess

import pytest

import hop_scenes as HS
import oracle_lib as O
import raytracer as rt
from raytracer import _native as N
from test_ground_hop import HOST, PKG, REPO, RT

SEED = 0x5EED
SEEDS = (SEED, 1, 7)
DRAWS = 300_000  # per stack

# ground stacks beyond tests/hop_scenes.py whose placement must leave the down pass out: a coat with nothing under
# it, and a coat whose only other member is a raised rect — its padded box makes the top plane, so it lies on Y
EXTRA = {
    "coat_only": lambda: [HS.coat(-HS.H, 0.0)] + HS.balls(0.0),
    "raised_only": lambda: [HS.coat(-HS.H, 0.0), HS.rect_xz(-1.5, -0.5, -0.5, 0.5, 0.5, HS.lambertian(0.9, 0.1, 0.1))]
    + HS.balls(0.5 + 2.0 ** -13),
}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("down_hop_check") / "down_hop_check")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-w", "-o", exe, os.path.join(REPO, "tests", "down_hop_check.c"),
                    "-lm", "-lpthread"], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def checks(checker, tmp_path_factory):
    """down_hop_check's counts on random_scene's primitives for three seeds and on every kind-2 stack of
    tests/hop_scenes.py, all at once (about a second each); the tied stacks under `ties`."""
    tmp = tmp_path_factory.mktemp("down_checks")
    procs = {}
    for seed in SEEDS:
        path = str(tmp / f"random_{seed}.prims")
        HS.write_prims(rt.scenes.random_scene(seed).finalize(seed), path)
        procs[f"random:{seed}"] = subprocess.Popen([checker, path, str(DRAWS), str(seed)], stdout=subprocess.PIPE,
                                                   stderr=subprocess.PIPE, text=True)
    for name in HS.KIND2:
        path = str(tmp / (name + ".prims"))
        HS.write_prims(HS.scene(name), path)
        procs[name] = subprocess.Popen([checker, path, str(DRAWS), "7"] + (["ties"] if name in HS.TIED else []),
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    res = {}
    for name, p in procs.items():
        out, err = p.communicate(timeout=600)
        print(f"{name}: rc {p.returncode} {out.strip()} {err.strip()}")
        res[name] = (p.returncode, json.loads(out))
    return res


@pytest.mark.parametrize("name", [f"random:{s}" for s in SEEDS] + HS.KIND2)
def test_no_found_or_served_ray_differs(checks, name):
    """300 000 adversarial draws per stack: no served and no found ray differs from the reference's own walk in
    primitive, face or t; on a tie-free stack neither differs from the exhaustive answer under both test orders.
    The draws do reach both outcomes, upward found hits (the rect from inside a lower box) included where the stack
    has them.  The controls — found hits that would differ with the "plane below Y" condition or the slope bounds
    switched off — are printed by the fixture; measured on this CPU: see profiles/downhop/README.md."""
    rc, r = checks[name]
    assert r["ground_stack"] == 1 and r["draws"] == DRAWS and r["hop_down"] == 1
    assert r["served_wrong_reference"] == 0 and r["found_wrong_reference"] == 0 and rc == 0
    if name not in HS.TIED:
        assert r["served_wrong"] == 0 and r["found_wrong"] == 0
    # (the draws do reach both outcomes: about one in five is served and one in twenty found on a tie-free stack.  In
    # a tied stack the rect shares a plane with a box face or the coat is there twice, so nearly every hit below the
    # coat carries a tie mark and is left to the traversal: no floor for `found` there)
    assert r["served"] > DRAWS // 40 and (name in HS.TIED or r["found"] > DRAWS // 100)


FRAME_W, FRAME_H = 64, 48
OPEN_XZ = (2.0, 2.0)  # tests/test_gpu_hop.py ground_camera's patch of ground between random_scene's spheres


def random_cameras():
    """The cameras of tests/test_gpu_downhop.py's random_scene frames (it takes them from here): tests/hop_scenes.py
    cameras() — down from 1.25 above, low from 7 degrees at 0.875 — on a 64x48 frame looking at OPEN_XZ on
    random_scene's coat (y = 0)."""
    import numpy as np
    (x, z), e, w, h = OPEN_XZ, np.radians(7.0), FRAME_W, FRAME_H
    down = rt.CameraBuilder(width=w, aspect_ratio=(w, h), vfov=30.0, focal_length=1.0, aperture=0.001).build(
        rt.CameraPosition((x, 1.25, z), (x, 0.0, z), (0.0, 0.0, -1.0), focus_length=1.25))
    low = rt.CameraBuilder(width=w, aspect_ratio=(w, h), vfov=8.0, focal_length=1.0, aperture=0.001).build(
        rt.CameraPosition((x + 0.875 * np.cos(e), 0.875 * np.sin(e), z), (x, 0.0, z), (0.0, 1.0, 0.0), focus_length=0.875))
    assert (down.image_width, down.image_height, low.image_width, low.image_height) == (w, h, w, h)
    return {"down": down, "low": low}


def test_random_scene_frames_hold_down_candidates():
    """The 64x48 frames tests/test_gpu_downhop.py renders of random_scene do run the down pass: by the oracle alone, in
    at least half of a frame's 48 tiles (a tile is a wave) 40 or more of the 64 sample-0 primary rays have the top
    face of the glass coat as their closest hit — the first run needs 32 such lanes, and the samples jitter."""
    sc = rt.scenes.random_scene(SEED).finalize(SEED)
    osc = O.OracleScene(sc)
    d = sc.desc
    for cam_name, cam in random_cameras().items():
        tiles = [[0] * 8 for _ in range(6)]
        for py in range(48):
            for px in range(64):
                ray = O._d6()
                O.lib().or_pixel_ray(cam, SEED, px, py, 0, ray)
                h = osc.hit(list(ray))
                if not h.hit:
                    continue
                o = d.objects[h.object]
                tiles[py // 8][px // 8] += (o.geometry == N.RT_GEOM_RECT_BOX and d.materials[o.material].kind == N.RT_MAT_DIELECTRIC
                                            and bool(h.front_face) and h.normal[1] == 1.0 and ray[4] < 0.0)
        n = sum(c >= 40 for row in tiles for c in row)
        print(f"random_scene {cam_name}: {n} of 48 tiles")
        assert n >= 24, cam_name


@pytest.fixture(scope="module")
def placements(tmp_path_factory):
    """tools/ground_stack on random_scene, every scene of tests/hop_scenes.py and EXTRA, under no variable and
    under SHIRLEY_HOP=up."""
    tmp = tmp_path_factory.mktemp("down_placements")
    exe = str(tmp / "ground_stack")
    flags = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter"]
    srcs = [os.path.join(REPO, "tools", "ground_stack.cpp"), os.path.join(RT, "scene_compile.cpp"),
            os.path.join(RT, "bvh_build.cpp")] + [os.path.join(HOST, f) for f in ("scene.cpp", "scenes.cpp", "host_api.cpp",
                                                                                 "earth_embed.S")]
    subprocess.run(["g++"] + flags + ["-Wa,-I," + os.path.join(PKG, "assets"), "-o", exe] + srcs + ["-lz", "-ldl"], check=True,
                   timeout=900)
    texts = {name: HS.scene_json(name) for name in HS.NAMES}
    texts.update({name: json.dumps({"skybox": "Above", "objects": objs()}) for name, objs in EXTRA.items()})
    cases = ["random", "random/HOP=up"]
    for name, text in texts.items():
        path = str(tmp / (name + ".json"))
        with open(path, "w") as f:
            f.write(text)
        cases += ["@" + path, "@" + path + "/HOP=up"]
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


@pytest.mark.parametrize("name", ["random"] + HS.NAMES + list(EXTRA))
def test_hop_down_follows_the_stack(placements, name):
    """hop_down is set exactly for the ground stacks with a non-dielectric member at least `gap` below the top plane
    (every kind-2 scene of tests/hop_scenes.py has the grey rect under its coat; EXTRA's two have none that
    qualifies; a scene without a ground stack has no down pass), never under SHIRLEY_HOP=up; hop_kind is what it was
    under both."""
    kind = 2 if name in ("random", *EXTRA) else HS.KIND[name]
    want = 1 if kind == 2 and name not in EXTRA else 0
    for mode in ("default", "up"):
        r = placements[name, mode]
        assert (r["hop_pass"], r["hop_kind"], r["stats_hop_kind"]) == (1, kind, kind), mode
        assert r["hop_down"] == (0 if mode == "up" else want), mode
