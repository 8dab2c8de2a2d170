"""The hop pass on synthetic ground stacks (tests/hop_scenes.py; trace.hip steps 5 and 5', rt_device.h ground_hop and
traverse4_root, scene_compile.cpp ground_stack): one small scene per premise of the proof the pass
serves by — a top plane off zero, no guarded sphere (no bitmap to read), a never-hit sphere, two glass boxes of
different index, a coat smaller than its rect, a top plane that is a rect's padded box, exact ties inside the stack
— and four scenes the compiler must leave to the first-node pass.  Frames are 32x32 @ 4 spp, sample_chunk 4 (the
oracle's in-order sums), seed 0x5EED, from two cameras that put whole waves on the coat
(tests/test_ground_hop.py test_frames_hold_hop_candidates).

  * the three uploads (ground stack, SHIRLEY_HOP=root, SHIRLEY_NO_HOP=1) give bit-identical frames and counters;
  * the default upload's frame meets the oracle's parity rule, each comparison with its own floor;
  * with the libm shared between device and oracle (the diagnostic builds) every channel is bit-identical: one
    flipped tie or one wrongly served hop fails that.

Measured: the module's 36 tests in 23.6 s, 22.4 s of it the session's device start; the shared-libm child 0.6 s, every
other test under 0.05 s."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hop_scenes as HS
import oracle_lib as O
import raytracer as rt
from test_gpu_hop_ground import render_modes, upload
from test_gpu_parity import PARITY_EXACT, check_parity

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "shirley-raytracing-rs_amd")
SEED = HS.SEED
SPP = 4
CAMS = ("down", "low")
# Per-comparison floors of the bit-identical fraction, min(0.9995, measured - 0.001) and never below PARITY_EXACT
# (tests/test_gpu_parity.py), from profiles/hopscenes/parity_fractions.jsonl: all 38 comparisons measured 1.0 (solid
# textures only), so every floor is 0.9995 and none is named here.
EXACT_FLOOR = {}


def exact_floor(key):
    return max(PARITY_EXACT, EXACT_FLOOR.get(key, 0.9995))


_scenes, _oracle = {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = HS.scene(name)
    return _scenes[name]


def oracle_frame(name, cam_name):
    """The oracle's frame at depth 50, computed once per scene and camera and never written to."""
    if (name, cam_name) not in _oracle:
        ora, _ = O.OracleScene(scene(name)).render(HS.cameras(name)[cam_name], O.params(SPP, 50, SEED), threads=16)
        ora.setflags(write=False)
        _oracle[name, cam_name] = ora
    return _oracle[name, cam_name]


def settings(depth=50, chunk=SPP):
    return rt.RenderSettings(samples=SPP, max_reflect=depth, seed=SEED, sample_chunk=chunk)


@pytest.mark.parametrize("name", HS.KIND2)
def test_modes_agree_on_a_ground_stack(gpu, monkeypatch, name):
    """Ground stack (1, 2), first node (1, 1) and no pass (0, 0): bit-identical frames, equal samples and segments.
    slab0 and two_coats also at depths 1, 2 and 3 and in units of one sample, where a path dies inside the first or
    the second run of the pass."""
    cams = HS.cameras(name)
    what = [(c, 50, SPP) for c in CAMS]
    if name in ("slab0", "two_coats"):
        what = [(c, depth, chunk) for c in CAMS for depth in (1, 2, 3, 50) for chunk in (1, SPP)]
    res = render_modes(gpu, monkeypatch, scene(name), [(cams[c], settings(depth, chunk)) for c, depth, chunk in what])
    for k, w in enumerate(what):
        a, a_samples, a_segments = res["ground"][k]
        for other in ("root", "off"):
            b, b_samples, b_segments = res[other][k]
            assert np.array_equal(a, b), (name, w, other)
            assert a_samples == b_samples == 32 * 32 * SPP, (name, w, other)
            assert a_segments == b_segments, (name, w, other)


@pytest.mark.parametrize("name", HS.KIND1)
def test_first_node_pass_chosen_by_the_compiler(gpu, monkeypatch, name):
    """A scene with no ground stack — a sphere's box starting below the top plane, a rect of another orientation,
    five ground primitives, a guard bitmap beyond its limit — uploads as (1, 1) by the compiler's own choice, and
    renders what no pass renders."""
    cams = HS.cameras(name)
    res = {}
    for mode, kind in (("ground", (1, 1)), ("off", (0, 0))):  # ("ground": the default upload, nothing set)
        assert upload(gpu, monkeypatch, scene(name), mode) == kind, (name, mode)
        res[mode] = []
        for c in CAMS:
            img = gpu.render(cams[c], settings())
            cnt = gpu.counters()
            res[mode].append((img, int(cnt.samples), int(cnt.segments)))
    for k, c in enumerate(CAMS):
        assert np.array_equal(res["ground"][k][0], res["off"][k][0]), (name, c)
        assert res["ground"][k][1:] == res["off"][k][1:], (name, c)
        assert res["ground"][k][1] == 32 * 32 * SPP


PARITY = [(name, "reference") for name in HS.NAMES] + [(name, "sah") for name in HS.TIED]


@pytest.mark.parametrize("name,bvh", PARITY)
def test_default_upload_matches_the_oracle(gpu, monkeypatch, name, bvh):
    """tests/test_gpu_parity.py check_parity on the default upload's frames, both cameras; the stacks with exact ties
    under both builders (the winner of a tie must not depend on the tree the device walks: DESIGN.md §8)."""
    monkeypatch.delenv("SHIRLEY_NO_HOP", raising=False)
    monkeypatch.delenv("SHIRLEY_HOP", raising=False)
    gpu.upload(scene(name), bvh=bvh)
    st = gpu.stats()
    assert (st.hop_pass, st.hop_kind) == (1, HS.KIND[name])
    for c, cam in HS.cameras(name).items():
        img = gpu.render(cam, settings())
        ora = oracle_frame(name, c)
        print(f"{name} {bvh} {c}: bit-identical channels {np.mean(img == ora):.5f}, max |gpu - oracle| "
              f"{np.abs(img - ora).max():.3g}")
        check_parity(img, ora, SPP, frac_exact=exact_floor(f"{name}:{bvh}:{c}"))


CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import raytracer as rt, oracle_lib as O, hop_scenes as HS
out = {}
dev = rt.Device(0)
for name, bvh in json.loads(sys.argv[3]):
    scene = HS.scene(name)
    dev.upload(scene, bvh=bvh)
    st = dev.stats()
    assert (st.hop_pass, st.hop_kind) == (1, HS.KIND[name]), name
    osc = O.OracleScene(scene)
    for c, cam in HS.cameras(name).items():
        img = dev.render(cam, rt.RenderSettings(samples=4, max_reflect=50, seed=HS.SEED, sample_chunk=4))
        ora, _ = osc.render(cam, O.params(4, 50, HS.SEED), threads=16)
        out[f"{name}:{bvh}:{c}"] = float(np.mean(img == ora))
dev.close()
print(json.dumps(out))
"""


def test_frames_are_bit_identical_with_a_shared_libm():
    """tests/test_gpu_libm_isolation.py's builds (lib/diag/libshirley_rt.so and oracle/liboracle_pl.so call the same
    portable functions) in one child process: every scene, camera and — for the tied stacks — builder, every
    channel bit-identical."""
    diag_lib = os.path.join(PKG, "lib", "diag")
    diag_oracle = os.path.join(REPO, "oracle", "liboracle_pl.so")
    assert os.path.exists(os.path.join(diag_lib, "libshirley_rt.so")) and os.path.exists(diag_oracle), \
        "diagnostic builds missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if k not in ("SHIRLEY_NO_HOP", "SHIRLEY_HOP")}
    env.update(SHIRLEY_LIB_DIR=diag_lib, SHIRLEY_ORACLE_SO=diag_oracle, SHIRLEY_NO_TORCH="1")
    r = subprocess.run([sys.executable, "-c", CHILD, PKG, os.path.join(REPO, "tests"), json.dumps(PARITY)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    shared = json.loads(r.stdout.strip().splitlines()[-1])
    path = os.environ.get("SHIRLEY_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": "hop_scenes_shared_libm", "shared_libm": shared}) + "\n")
    print(json.dumps(shared))
    assert len(shared) == 2 * len(PARITY)
    for key, frac in shared.items():
        assert frac == 1.0, f"{key}: {frac} of channels bit-identical with the libm shared"
