"""The light-sampling path integrator on the CPU (include/shirley_rt.h, added within ABI 11): the
library exports the entry points, ray-cli names --nee and refuses what it cannot be combined with before any
device is opened, and the oracle restatement of the integrator (tests/nee_ref.py) is checked on its own: it is the
plain render where no light is listed and at max_depth = 1, and its expectation is the render's."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import direct_ref as D
import nee_ref as R
import oracle_lib as O
import raytracer as rt
from raytracer import _native as N

CLI = os.path.join(N.BIN_DIR, "ray-cli")
SEED = 0x5EED
NEE = ["render", "cornell", "-w", "64", "-s", "4", "--nee"]


def test_library_exports_the_two_symbols_within_abi_11():
    lib = N.rt_lib()
    for sym in ("rt_render_nee", "rt_render_nee_device"):
        assert sym in N.RT_SIGNATURES and getattr(lib, sym) is not None
    assert N.RT_NEE_MIS == 1
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "shirley_rt.h")) as f:
        text = f.read()
    assert "#define RT_ABI_VERSION 11" in text
    assert "int rt_render_nee(" in text and "int rt_render_nee_device(" in text and "RT_NEE_MIS = 1" in text


def test_usage_names_the_nee_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--nee" in r.stderr and "--nee-mis 0|1" in r.stderr


@pytest.mark.parametrize("extra,word", [(["--gpus", "2"], "one GPU"), (["--progressive", "2"], "--progressive"),
                                        (["--resume", "nowhere.f64"], "--resume"), (["--adaptive", "0.05"], "--adaptive"),
                                        (["--denoise"], "--denoise"), (["--ao", "1"], "--ao"),
                                        (["--direct"], "--direct"), (["--dump-accum", "nowhere.f64"], "--dump-accum")])
def test_nee_refuses_what_it_does_not_support(extra, word):
    r = subprocess.run([CLI] + NEE + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "error: --nee" in r.stderr and word in r.stderr


def test_nee_refuses_book2_scenes_before_a_device_is_opened():
    r = subprocess.run([CLI, "render", "final", "-w", "32", "-s", "1", "--nee"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1
    assert "error: --nee" in r.stderr and "book-2" in r.stderr and "rt_create" not in r.stderr


def test_a_bad_mis_value_is_a_usage_error():
    r = subprocess.run([CLI] + NEE + ["--nee-mis", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--nee-mis 0 or 1" in r.stderr
    r = subprocess.run([CLI] + NEE + ["--nee-mis"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "missing value for --nee-mis" in r.stderr


@pytest.mark.parametrize("mis", [False, True])
def test_restatement_without_a_listed_light_is_the_render(mis):
    """The day random scene lists no light: no vertex takes a sample and no hit is re-weighted, so the sums are
    or_render_rows' in-order sums (chunk >= samples), bit for bit, for both flag values."""
    sc = rt.scenes.random_scene(SEED).finalize(SEED)
    cam = rt.scene_camera("random", 16, "square")
    assert (cam.image_width, cam.image_height) == (16, 16)
    osc = O.OracleScene(sc)
    ref = R.oracle_nee(sc, cam, SEED, 0, 2, 8, mis, osc)
    ora, _ = osc.render(cam, O.params(2, 8, SEED, chunk=2))
    assert ref.sampled == 0 and ref.reweighted == 0 and ref.misses > 0 and ref.depth_cut > 0
    assert np.array_equal(ref.sums, ora)


@pytest.mark.parametrize("mis", [False, True])
def test_restatement_at_depth_1_is_the_render(mis):
    """max_depth = 1: the only vertex is the last one, which takes no sample."""
    sc = D.lambert_box().finalize(SEED)
    cam = rt.default_camera(16, "square")
    osc = O.OracleScene(sc)
    ref = R.oracle_nee(sc, cam, SEED, 0, 4, 1, mis, osc)
    ora, _ = osc.render(cam, O.params(4, 1, SEED, chunk=4))
    assert ref.sampled == 0 and ref.longest == 1 and ora.max() > 0.0
    assert np.array_equal(ref.sums, ora)


@pytest.mark.parametrize("depth", [2, 5])
def test_restatement_has_the_renders_expectation(depth):
    """direct_ref.lambert_box() at 16x16, K = 16 disjoint ranges of 8 spp, seed 0x5EED: the frame mean per sample
    and its standard error from the K range means, for or_render_rows and for the restatement with RT_NEE_MIS clear
    and set; |difference| <= 5 sqrt(se1^2 + se2^2) for both.  Measured:
      depth 2: render 0.164086 +- 0.003470, MIS clear 0.171315 +- 0.003456 (z 1.48), set 0.168796 +- 0.001212 (z 1.28)
      depth 5: render 0.194214 +- 0.002725, MIS clear 0.198129 +- 0.003527 (z 0.88), set 0.197906 +- 0.001290 (z 1.22)
    (z: the difference in combined standard errors; both depths take about 3 s together.)"""
    (m0, s0), (m1, s1), (m2, s2) = R.expectation_figures(R.box16, depth, 16, 8, SEED)
    for label, m, s in (("MIS clear", m1, s1), ("MIS set", m2, s2)):
        z = (m - m0) / math.hypot(s, s0)
        print(f"depth {depth}: render {m0:.6f} +- {s0:.6f}, {label} {m:.6f} +- {s:.6f} (z {z:.2f})")
        assert s > 0.0 and s0 > 0.0 and m > 0.0
        assert abs(m - m0) <= 5.0 * math.hypot(s, s0)
