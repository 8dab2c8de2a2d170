"""The light list and the direct-lighting pass on the CPU (include/shirley_rt.h, added within ABI 11): the
library exports the entry points, rt_scene_lights_host applies the listing rule to a hand-built scene and to the
built-in ones, ray-cli names --direct and refuses what it cannot be combined with before any device is opened,
and the oracle restatement of the pass (tests/direct_ref.py) meets every kind of sample on the Cornell box."""
import ctypes as C
import os
import subprocess

import pytest

import direct_ref as D
import raytracer as rt
from raytracer import _native as N

CLI = os.path.join(N.BIN_DIR, "ray-cli")
SEED = 0x5EED
DIRECT = ["render", "cornell", "-w", "64", "-s", "4", "--direct"]


def test_library_exports_the_four_symbols_within_abi_11():
    lib = N.rt_lib()
    for sym in ("rt_scene_lights", "rt_scene_lights_host", "rt_render_direct", "rt_render_direct_device"):
        assert sym in N.RT_SIGNATURES and getattr(lib, sym) is not None
    assert C.sizeof(N.rt_light) == 48
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "shirley_rt.h")) as f:
        text = f.read()
    assert "#define RT_ABI_VERSION 11" in text and "int rt_render_direct(" in text


def test_hand_built_scene_lists_its_lights_in_object_order():
    sc = D.hand_scene().finalize(SEED)
    lights, unlisted = D.host_lights(sc.desc)
    got = [(l.object, l.geometry, l.emitter, l.area, tuple(l.color)) for l in lights]
    assert got == D.HAND_LIGHTS  # areas and colours computed by hand (direct_ref.HAND_LIGHTS), exact
    assert unlisted == D.HAND_UNLISTED == 4
    # the restated rule agrees, and the counts-only call returns the same counts
    restated, u2 = D.list_lights(sc.desc)
    assert [(i, g, e, a, tuple(c)) for i, g, e, _, a, c in restated] == got and u2 == unlisted
    n, u = C.c_int32(-1), C.c_int32(-1)
    assert N.rt_lib().rt_scene_lights_host(C.byref(sc.desc), C.byref(n), C.byref(u), None) == N.RT_OK
    assert (n.value, u.value) == (5, 4)
    assert N.rt_lib().rt_scene_lights_host(None, C.byref(n), C.byref(u), None) == N.RT_E_INVALID


def test_built_in_light_counts():
    cornell, u = D.host_lights(rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED).desc)
    assert len(cornell) == 1 and u == 0
    assert (cornell[0].geometry, cornell[0].emitter) == (N.RT_GEOM_RECT_XZ, N.RT_MAT_FAIRY_LIGHT)
    assert cornell[0].area == 130.0 * 105.0
    day, u = D.host_lights(rt.scenes.random_scene(SEED).finalize(SEED).desc)
    assert len(day) == 0 and u == 0
    box, u = D.host_lights(rt.SceneBuilder.builtin("box-light", SEED).finalize(SEED).desc)
    assert [(l.geometry, l.emitter, l.area) for l in box] == [(N.RT_GEOM_RECT_XZ, N.RT_MAT_DIFFUSE_LIGHT, 4.0)]
    night, _ = D.host_lights(rt.scenes.random_scene(SEED, night=True).finalize(SEED).desc)
    assert len(night) > 1 and all(l.geometry == N.RT_GEOM_SPHERE and l.emitter == N.RT_MAT_FAIRY_LIGHT
                                  for l in night)


def test_usage_names_the_direct_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--direct" in r.stderr and "--direct-chain K" in r.stderr


@pytest.mark.parametrize("extra,word", [(["--gpus", "2"], "one GPU"), (["--progressive", "2"], "--progressive"),
                                        (["--resume", "nowhere.f64"], "--resume"), (["--adaptive", "0.05"], "--adaptive"),
                                        (["--denoise"], "--denoise"), (["--ao", "1"], "--ao"),
                                        (["--dump-accum", "nowhere.f64"], "--dump-accum")])
def test_direct_refuses_what_it_does_not_support(extra, word):
    r = subprocess.run([CLI] + DIRECT + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "error: --direct" in r.stderr and word in r.stderr


def test_direct_refuses_book2_scenes_before_a_device_is_opened():
    r = subprocess.run([CLI, "render", "final", "-w", "32", "-s", "1", "--direct"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1
    assert "error: --direct" in r.stderr and "book-2" in r.stderr and "rt_create" not in r.stderr


def test_missing_or_negative_chain_is_a_usage_error():
    r = subprocess.run([CLI, "render", "cornell", "--direct", "--direct-chain"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "missing value for --direct-chain" in r.stderr
    r = subprocess.run([CLI, "render", "cornell", "--direct", "--direct-chain", "-1"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--direct-chain K >= 0" in r.stderr


def test_restatement_meets_every_kind_of_sample_on_the_cornell_box():
    """Cornell box, cornell_camera(24), 2 spp, chain 0: every counter category the scene can produce is > 0 —
    misses, FairyLight emitter vertices, light samples (all on the one FairyLight xz_rect), back-face cuts,
    occluded and unoccluded shadow rays — and both buffers hold non-zero values."""
    sc = rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED)
    ref = D.oracle_direct(sc, rt.cornell_camera(24), SEED, 0, 2, 0)
    print(f"cornell: {ref.sampled} light samples {ref.kinds}, {ref.cut} cut, {ref.occluded} occluded, "
          f"{ref.unoccluded} unoccluded; {ref.fairy_light} emitter vertices, {ref.misses} misses")
    assert ref.misses > 0 and ref.fairy_light > 0 and ref.diffuse_light == 0
    assert ref.kinds == {(N.RT_GEOM_RECT_XZ, N.RT_MAT_FAIRY_LIGHT): ref.sampled} and ref.sampled > 500
    assert ref.cut > 0 and ref.occluded > 0 and ref.unoccluded > 0
    assert ref.cut + ref.occluded + ref.unoccluded == ref.sampled
    assert ref.most_attempts > 1  # (the Cornell camera has a lens)
    assert ref.emission.max() > 0.0 and ref.direct.max() > 0.0 and ref.direct.min() >= 0.0
    assert ref.solid.all()
