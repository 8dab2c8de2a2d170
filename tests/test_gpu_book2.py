"""Every book-2 primitive form on the device against the oracle (rt_device.h ext_t / base_t / ext_record / to_object,
leaf_tests4's inline and deferred object tests, ray_time / moving_center, the Isotropic scatter) on the
scenes of tests/book2_scenes.py, whose coverage tests/test_book2_scenes.py proves with the oracle alone: each base
shape as a surface, an instance, a medium and an instanced medium, 54 extended objects on both sides of DExt index
32, moving spheres whose interval is not the shutter's, rays that start inside media and boxes, axis-parallel rays
and rays cut by a finite t_max.

  * per-ray records of both traversals, in three node placements and under both builders: the object of every
    ray, surfaces bit for bit, media within an ulp of log;
  * Isotropic probes: scattered, the albedo, the hit point, the oracle's direction bit for bit;
  * twin scenes (a moving sphere frozen by the shutter against the static one, a shape under a null or an integer
    Transform against the bare shape): equal frames and counters, the extended kernel instance against the
    reference one;
  * frames against the oracle by test_gpu_parity.py's rule, floors from profiles/book2/parity_fractions.jsonl;
  * the kernel instances of a book-2 scene (wide and narrow block, material tables in LDS or not, both trees,
    the wavefront engine's two extend kernels, the adaptive tile lists): one frame, bit for bit;
  * with the libm shared between device and oracle (the diagnostic builds, one child process): every frame, every
    record and every probe bit-identical, so that a gap in the product run is an ulp of the libm or a defect.

Frames are 32x32 @ 8 spp, depth 16, seed 0x5EED."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import book2_scenes as B
import oracle_lib as O
import raytracer as rt
from raytracer import _native as N
from test_gpu_parity import PARITY_EXACT, check_parity

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "shirley-raytracing-rs_amd")
SEED = B.SEED
SPP, DEPTH = 8, 16
NAMES = ["zoo", "zoo_solid", "smoke", "many_ext", "shutter"]
PLACEMENTS = ["auto", "global", "half-lds"]
HIT = np.dtype(N.rt_hit)
PROBE = np.dtype(N.rt_probe)
SWAPS = 0.001  # share of a set's rays on which an ulp of log may swap a medium's scatter with what lies just behind
# Per-comparison floors of the bit-identical fraction, min(0.9995, measured - 0.001) and never below PARITY_EXACT
# (tests/test_gpu_parity.py), from profiles/book2/parity_fractions.jsonl; a frame that is not named measured 1.0.
EXACT_FLOOR = {}
FRAMES = ["zoo", "zoo_solid", "smoke", "many_ext", "shutter:open", "shutter:inner", "shutter:frozen"]


def exact_floor(key):
    return max(PARITY_EXACT, EXACT_FLOOR.get(key, 0.9995))


def settings(**kw):
    return rt.RenderSettings(**{**dict(samples=SPP, max_reflect=DEPTH, seed=SEED, sample_chunk=SPP), **kw})


def frame_inputs(key):
    """(scene, camera) of FRAMES' key."""
    if key.startswith("shutter:"):
        return B.get("shutter")[0], B.shutter(key.split(":")[1])[1]
    return B.get(key)[:2]


_oracle_frames = {}


def oracle_frame(key):
    if key not in _oracle_frames:
        scene, cam = frame_inputs(key)
        ora, cnt = O.OracleScene(scene).render(cam, O.params(SPP, DEPTH, SEED), threads=16)
        ora.setflags(write=False)
        _oracle_frames[key] = (ora, int(cnt.samples))
    return _oracle_frames[key]


# ---- per-ray records --------------------------------------------------------------------------------------------

def device_hits(dev, rays, t_max, traversal):
    hits = dev.hit(rays, B.T_MIN, t_max, traversal=traversal)
    return np.frombuffer(b"".join(bytes(h) for h in hits), dtype=HIT)


def media_of(scene):
    """is_medium[object + 1] (index 0: no object)."""
    return np.array([False] + [bool(o.medium) for o in B.objects(scene)])


def same_bits(g, h):
    """_same_record of tests/test_gpu_traversal.py on arrays: t, point, normal, front_face."""
    return ((g["t"] == h["t"]) & np.all(g["point"] == h["point"], axis=1) & np.all(g["normal"] == h["normal"], axis=1)
            & ((g["front_face"] != 0) == (h["front_face"] != 0)))


def record_stats(scene, g, h):
    """Device records g against the oracle's h (or_hit) of one ray set, as counts of rays.  A medium's normal is
    constant_medium.h's arbitrary (1, 0, 0) — rotated with the instance, where the medium is one — so the oracle's
    bit for bit; its t and point carry the free flight's log."""
    med = media_of(scene)
    want = np.where(h["hit"] != 0, h["object"], -1)
    differ = g["object"] != want
    same = ~differ & (want >= 0)
    m = same & med[want + 1]
    s = same & ~med[want + 1]
    bits = same_bits(g, h)
    with np.errstate(invalid="ignore"):
        medium_ok = ((np.abs(g["t"] - h["t"]) <= 1e-13 * np.abs(h["t"]))
                     & np.all(np.isclose(g["point"], h["point"], rtol=1e-12, atol=1e-9), axis=1)
                     & np.all(g["normal"] == h["normal"], axis=1) & (g["front_face"] != 0) & (h["front_face"] != 0))
        uv_ok = (np.abs(g["u"] - h["u"]) < 1e-12) & (np.abs(g["v"] - h["v"]) < 1e-12)
    return {"n": len(g), "hits": int(same.sum()), "media": int(m.sum()), "differ": int(differ.sum()),
            "differ_off_media": int((differ & ~(med[want + 1] | med[g["object"] + 1])).sum()),
            "surface_bad": int((s & ~bits).sum()), "medium_bad": int((m & ~medium_ok).sum()),
            "medium_bits_bad": int((m & ~bits).sum()), "uv_bad": int((same & ~uv_ok).sum())}


def check_records(st, where, shared_libm=False):
    assert st["differ_off_media"] == 0, (where, st)
    assert st["surface_bad"] == 0 and st["uv_bad"] == 0 and st["medium_bad"] == 0, (where, st)
    if shared_libm:
        assert st["differ"] == 0 and st["medium_bits_bad"] == 0, (where, st)
    else:
        assert st["differ"] <= SWAPS * st["n"], (where, st)


@pytest.mark.parametrize("nodes", PLACEMENTS)
@pytest.mark.parametrize("bvh", ["reference", "sah"])
@pytest.mark.parametrize("name", NAMES)
def test_hit_records_match_the_oracle(gpu, name, bvh, nodes):
    """rt_scene_hit (the 2-wide f64 tree) and rt_scene_hit_ex(RT_TRAVERSAL_RENDER) (the traversal the trace kernels
    run: leaf_tests4 with the deferred and the inline extended-object test) on every ray set: the oracle's object for
    every ray — but where an ulp of log swaps a medium's scatter with its neighbour, on at most 0.1 % of a set —
    surfaces' records bit for bit, u and v within 1e-12, media within 1e-13 relative in t; and the two traversals
    agree record for record."""
    scene, _, sets = B.get(name)
    want = B.oracle_hits(name)
    gpu.upload(scene, bvh, nodes)
    total = {"hits": 0, "media": 0}
    for s, (rays, t_max) in sets.items():
        got = {tv: device_hits(gpu, rays, t_max, tv) for tv in ("binary", "render")}
        for tv, g in got.items():
            st = record_stats(scene, g, want[s])
            check_records(st, (name, bvh, nodes, s, tv))
            total = {k: total[k] + st[k] for k in total}
        a, b = got["binary"], got["render"]
        assert np.array_equal(a["object"], b["object"]), (name, s)
        assert same_bits(a, b)[a["object"] >= 0].all(), (name, s)
    assert total["hits"] >= 1500 and (total["media"] >= 400 or name not in ("smoke", "many_ext"))


# ---- Isotropic probes -------------------------------------------------------------------------------------------

PROBE_SETS = ("camera", "objects", "from_inside")
PROBE_DRAWS = (0, 3, 7)
PROBE_SAMPLE = 2
_oracle_probes = {}


def probe_rays():
    sets = B.get("smoke")[2]
    return np.vstack([sets[s][0] for s in PROBE_SETS])


def oracle_probes(draw):
    if draw not in _oracle_probes:
        osc = O.OracleScene(B.get("smoke")[0])
        rec = b"".join(bytes(osc.probe(r, SEED, i, PROBE_SAMPLE, draw)) for i, r in enumerate(probe_rays()))
        _oracle_probes[draw] = np.frombuffer(rec, dtype=PROBE)
    return _oracle_probes[draw]


def device_probes(dev, draw):
    out = dev.probe(probe_rays(), SEED, PROBE_SAMPLE, draw)
    return np.frombuffer(b"".join(bytes(p) for p in out), dtype=PROBE)


def albedos(scene):
    """[object + 1][3]: the solid colour of each object's texture."""
    d = scene.desc
    return np.array([[0.0, 0.0, 0.0]] + [list(d.textures[d.materials[o.material].texture].color) for o in B.objects(scene)])


def probe_stats(scene, g, h):
    med = media_of(scene)
    differ = g["object"] != h["object"]
    same = ~differ & (h["object"] >= 0)
    m = same & med[h["object"] + 1]
    eq3 = lambda a, b: np.all(a == b, axis=1)  # noqa: E731
    with np.errstate(invalid="ignore"):
        t_ok = np.abs(g["t"] - h["t"]) <= 1e-13 * np.abs(h["t"])
    per_medium = np.bincount(h["object"][m], minlength=len(med) - 1)
    return {"n": len(g), "media": int(m.sum()), "differ": int(differ.sum()),
            "differ_off_media": int((differ & ~(med[h["object"] + 1] | med[g["object"] + 1])).sum()),
            "per_medium": [int(per_medium[i]) for i in range(len(med) - 1) if med[i + 1]],
            "not_scattered": int((m & (g["scattered"] != 1)).sum()),
            "attenuation_bad": int((m & ~eq3(g["attenuation"], albedos(scene)[g["object"] + 1])).sum()),
            "origin_bad": int((m & ~eq3(g["origin"], g["point"])).sum()),
            "direction_bad": int((m & ~eq3(g["direction"], h["direction"])).sum()),
            "draw_bad": int((same & (g["draw"] != h["draw"])).sum()),
            "scatter_flag_bad": int((same & (g["scattered"] != h["scattered"])).sum()),
            "t_bad": int((m & ~t_ok).sum()),
            "bits_bad": int((same & ~((g["t"] == h["t"]) & eq3(g["point"], h["point"]) & eq3(g["normal"], h["normal"])
                                      & eq3(g["direction"], h["direction"]) & eq3(g["origin"], h["origin"]))).sum())}


def check_probes(st, where, shared_libm=False):
    assert st["differ_off_media"] == 0, (where, st)
    for k in ("not_scattered", "attenuation_bad", "origin_bad", "direction_bad", "draw_bad", "scatter_flag_bad", "t_bad"):
        assert st[k] == 0, (where, k, st)
    if shared_libm:
        assert st["differ"] == 0 and st["bits_bad"] == 0, (where, st)
    else:
        assert st["differ"] <= SWAPS * st["n"], (where, st)


def test_isotropic_probes_match_the_oracle(gpu):
    """rt_probe_segment on rays into the smoke scene's media, at three draw indices (the free flight and the
    scatter draw from them): a medium's hit scatters, attenuates by its albedo, leaves from the hit point in the
    oracle's direction (random_in_unit_sphere on the path's stream) bit for bit, and uses the oracle's draws."""
    scene = B.get("smoke")[0]
    gpu.upload(scene)
    per_medium = None
    for draw in PROBE_DRAWS:
        st = probe_stats(scene, device_probes(gpu, draw), oracle_probes(draw))
        check_probes(st, draw)
        per_medium = st["per_medium"] if per_medium is None else [a + b for a, b in zip(per_medium, st["per_medium"])]
    # (the last medium is the rect boundary, which never scatters)
    assert per_medium[-1] == 0 and min(per_medium[:-1]) >= 50, per_medium


# ---- twins ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", B.TWINS)
def test_twins_render_equal_frames(gpu, key):
    """Frames and path counters of a scene and its twin are equal (tests/book2_scenes.py twin; on the oracle:
    tests/test_book2_scenes.py): the extended side runs ext_t / ext_record in the EXT kernel instance (a sphere
    under a null rotation is flattened at upload instead), its twin the reference instance."""
    ext, bare, cam = B.twin(key)
    s = settings(samples=4, sample_chunk=4, engine="megakernel")
    a = gpu.upload(ext).render(cam, s)
    ca = gpu.counters()
    b = gpu.upload(bare).render(cam, s)
    cb = gpu.counters()
    assert np.array_equal(a, b), f"{np.mean(a != b):.4f} of channels differ"
    assert (ca.samples, ca.segments) == (cb.samples, cb.segments) and ca.samples == 32 * 32 * 4
    assert ca.engine == cb.engine == 1


# ---- frames -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", FRAMES)
def test_frames_match_the_oracle(gpu, key):
    scene, cam = frame_inputs(key)
    ora, samples = oracle_frame(key)
    img = gpu.upload(scene).render(cam, settings())
    print(f"{key}: bit-identical channels {np.mean(img == ora):.5f}, max |gpu - oracle| {np.abs(img - ora).max():.3g}")
    assert gpu.counters().samples == samples == 32 * 32 * SPP
    check_parity(img, ora, SPP, frac_exact=exact_floor(key))


@pytest.mark.parametrize("name", ["smoke", "many_ext"])
def test_kernel_instances_render_one_frame(gpu, monkeypatch, name):
    """The wide block and SHIRLEY_NO_WIDE's 256-thread instances, the material tables out of LDS
    (SHIRLEY_NO_LDS_MATS), the reference and the SAH tree, the wavefront engine with wf_extend4 and with wf_extend
    (SHIRLEY_WF_EXTEND2), and render_adaptive at threshold 0 (4 samples for every pixel, then a step of 4 for every
    tile through the tile-list instance): one frame, bit for bit.  In units of 2 samples, the adaptive batch."""
    scene, cam, _ = B.get(name)
    s = dict(samples=SPP, sample_chunk=2)
    flags = ("SHIRLEY_NO_WIDE", "SHIRLEY_NO_LDS_MATS", "SHIRLEY_WF_EXTEND2")
    for f in flags:
        monkeypatch.delenv(f, raising=False)
    base = gpu.upload(scene).render(cam, settings(**s))
    assert np.isfinite(base).all() and base.max() > 0
    frames = {}
    for f in flags[:2]:
        monkeypatch.setenv(f, "1")
        frames[f] = gpu.upload(scene).render(cam, settings(**s))
        monkeypatch.delenv(f)
    frames["sah"] = gpu.upload(scene, "sah").render(cam, settings(**s))
    frames["wavefront"] = gpu.upload(scene).render(cam, settings(**s, engine="wavefront"))
    assert gpu.counters().engine == 2
    monkeypatch.setenv(flags[2], "1")
    frames["wavefront, wf_extend"] = gpu.upload(scene).render(cam, settings(**s, engine="wavefront"))
    assert gpu.counters().engine == 2
    monkeypatch.delenv(flags[2])
    gpu.upload(scene)
    accum, counts, _, _, rep = gpu.render_adaptive(cam, settings(**s), rt.AdaptiveSettings(threshold=0.0, min_samples=4, step=4))
    assert (counts == SPP).all() and rep.steps == 2
    frames["adaptive"] = accum
    for k, img in frames.items():
        assert np.array_equal(img, base), f"{name}, {k}: {np.mean(img != base):.4f} of channels differ"


# ---- the libm shared --------------------------------------------------------------------------------------------

def child_main():
    """Runs in the child process of test_everything_is_bit_identical_with_a_shared_libm: every comparison above that
    involves the oracle, as counts."""
    out = {"frames": {}, "records": {}, "probes": {}}
    dev = rt.Device(0)
    for key in FRAMES:
        scene, cam = frame_inputs(key)
        img = dev.upload(scene).render(cam, settings())
        out["frames"][key] = float(np.mean(img == oracle_frame(key)[0]))
    for name in NAMES:
        scene, _, sets = B.get(name)
        want = B.oracle_hits(name)
        dev.upload(scene)
        for s, (rays, t_max) in sets.items():
            for tv in ("binary", "render"):
                out["records"][f"{name}:{s}:{tv}"] = record_stats(scene, device_hits(dev, rays, t_max, tv), want[s])
    scene = B.get("smoke")[0]
    dev.upload(scene)
    for draw in PROBE_DRAWS:
        out["probes"][str(draw)] = probe_stats(scene, device_probes(dev, draw), oracle_probes(draw))
    dev.close()
    print(json.dumps(out))


CHILD = "import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2]); import test_gpu_book2 as T; T.child_main()"


def test_everything_is_bit_identical_with_a_shared_libm():
    """tests/test_gpu_libm_isolation.py's builds (lib/diag/libshirley_rt.so and oracle/liboracle_pl.so call the same
    portable log, sin, acos and atan2) in one child process: every frame above 1.0 identical, every per-ray record —
    media included — and every probe bit-identical, and the object of no ray differs."""
    diag_lib = os.path.join(PKG, "lib", "diag")
    diag_oracle = os.path.join(REPO, "oracle", "liboracle_pl.so")
    assert os.path.exists(os.path.join(diag_lib, "libshirley_rt.so")) and os.path.exists(diag_oracle), \
        "diagnostic builds missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if k not in ("SHIRLEY_NO_WIDE", "SHIRLEY_NO_LDS_MATS", "SHIRLEY_WF_EXTEND2")}
    env.update(SHIRLEY_LIB_DIR=diag_lib, SHIRLEY_ORACLE_SO=diag_oracle, SHIRLEY_NO_TORCH="1")
    r = subprocess.run([sys.executable, "-c", CHILD, PKG, os.path.join(REPO, "tests")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    shared = json.loads(r.stdout.strip().splitlines()[-1])
    path = os.environ.get("SHIRLEY_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": "book2_shared_libm", "shared_libm": shared}) + "\n")
    print(json.dumps(shared["frames"]))
    assert sorted(shared["frames"]) == sorted(FRAMES) and len(shared["records"]) == 2 * 6 * len(NAMES)
    for key, frac in shared["frames"].items():
        assert frac == 1.0, f"{key}: {frac} of channels bit-identical with the libm shared"
    for key, st in shared["records"].items():
        check_records(st, key, shared_libm=True)
    for key, st in shared["probes"].items():
        check_probes(st, key, shared_libm=True)
