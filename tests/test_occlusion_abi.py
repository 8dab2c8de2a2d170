"""ABI 11 on the CPU: the library exports the occlusion entry points, ray-cli names --ao and refuses what it
cannot be combined with before any device is opened, and the oracle restatement of the ambient-occlusion pass
(tests/ao_ref.py) forms, at every Lambertian vertex, the very direction the oracle's own scatter returns."""
import os
import subprocess

import pytest

import ao_ref
import raytracer as rt
from raytracer import _native as N

CLI = os.path.join(N.BIN_DIR, "ray-cli")
SEED = 0x5EED
AO = ["render", "random", "-w", "64", "-s", "4", "--ao", "1"]


def test_library_exports_the_four_symbols():
    lib = N.rt_lib()
    for sym in ("rt_scene_occluded", "rt_scene_occluded_device", "rt_render_ao", "rt_render_ao_device"):
        assert sym in N.RT_SIGNATURES and getattr(lib, sym) is not None
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "shirley_rt.h")) as f:
        assert "#define RT_ABI_VERSION 11" in f.read()


def test_usage_names_the_ao_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--ao RADIUS" in r.stderr and "--ao-chain K" in r.stderr


@pytest.mark.parametrize("extra,word", [(["--gpus", "2"], "one GPU"), (["--progressive", "2"], "--progressive"),
                                        (["--resume", "nowhere.f64"], "--resume"), (["--adaptive", "0.05"], "--adaptive"),
                                        (["--denoise"], "--denoise")])
def test_ao_refuses_what_it_does_not_support(extra, word):
    r = subprocess.run([CLI] + AO + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "error: --ao" in r.stderr and word in r.stderr


@pytest.mark.parametrize("value", ["0", "-1", "nan", "radius"])
def test_ao_radius_must_be_positive(value):
    r = subprocess.run([CLI, "render", "random", "--ao", value], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--ao takes a radius > 0" in r.stderr


def test_ao_refuses_book2_scenes_before_a_device_is_opened():
    r = subprocess.run([CLI, "render", "final", "-w", "32", "-s", "1", "--ao", "inf"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1
    assert "error: --ao" in r.stderr and "book-2" in r.stderr and "rt_create" not in r.stderr


def test_missing_value_is_a_usage_error():
    r = subprocess.run([CLI, "render", "random", "--ao"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "missing value for --ao" in r.stderr


def test_restated_direction_is_the_oracles_own_scatter():
    """Cornell box, cornell_camera(40), 2 spp, chain 0: at every Lambertian feature vertex ao_ref's direction
    equals or_probe_segment's, component for component."""
    sc = rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED)
    ref = ao_ref.oracle_ao(sc, rt.cornell_camera(40), SEED, 0, 2, 0, 300.0)
    print(f"cornell: {ref.same} of {ref.lambertian} Lambertian vertices identical; {ref.vertices} vertices, "
          f"{ref.occluded} occluded, {ref.misses} misses")
    assert ref.lambertian > 2000 and ref.same == ref.lambertian
    assert ref.vertices + ref.misses == 40 * 40 * 2
    assert ref.occluded > 0 and ref.vertices - ref.occluded > 0 and ref.misses > 0
