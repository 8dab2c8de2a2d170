"""Every kernel instance the placement plan can select (the instance table), run through every entry
point that dispatches on it.

The plan (csrc/rt/scene_compile.cpp plan_placement) picks per scene the block (1024 / 768 threads, or 256) and where
the 4-wide tree, the primitives, the material and texture tables and the Perlin tables live (MODE = kSceneLds /
kNodesLds / kNodesGlobal / kNodesMixed); tests/test_scene_plan.py pins that choice on the CPU for every upload-time
switch.  Here the kernels those plans select run on the device.  The contract: a placement moves data, it never
changes a bit.  So each case uploads a scene under a plan other than its default one, runs an entry point, and
compares with the same call under the default plan of the same scene and builder, bit for bit; and once per scene
and pass the default plan's result is compared with the CPU oracle (or the pass's restatement) by the helper of the
pass's own test module, which ties every variant to the high-precision reference.

Frames are 40-48 pixels wide, max depth 50, at 4 spp; the frames of rt_render and rt_render_adaptive, which are
compared with the oracle by check_parity and the scene's EXACT_FLOOR entry, have that entry's own size (the frames of
test_render_matches_oracle: 8 spp; at 4 spp the 48-wide random_scene frame measures 0.9946, as __graft_entry__.smoke
records, under its 8-spp floor of 0.99566).  Ray batches hold 2048 rays.
"""
import contextlib
import json
import os

import numpy as np
import pytest

import ao_ref
import direct_ref as D
import lightgrid_ref as G
import lightvis_ref as V
import nee_ref as R
import oracle_lib as O
import raytracer as rt
import rect_ref as RR
from raytracer import _native as N
from test_gpu_features import check as check_features
from test_gpu_features import oracle_features
from test_gpu_light_rect import parity as parity_where_solid
from test_gpu_occlusion import oracle_occluded
from test_gpu_parity import check_parity, exact_floor
from test_gpu_traversal import _check_against_oracle, _same_record, random_scene_rays, scene_box_rays

pytestmark = pytest.mark.gpu

SEED = 0x5EED
SPP, DEPTH, N_RAYS = 4, 50, 2048
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "scene_plan.json")
SWITCHES = ("NO_WIDE", "NO_LDS_PRIMS", "NO_LDS_MATS", "NO_LDS_PERLIN", "LDS_NODES")

# scene -> (camera scene, width, aspect, EXACT_FLOOR key, AO radius, spp of the frames compared by that floor)
SCENES = {
    "spheres:4": ("spheres", 48, "std16x9", "spheres", 0.5, 4),
    "random": ("random", 48, "std16x9", "random", 0.5, 8),
    "random-night": ("random", 48, "std16x9", "random-night", 0.5, 8),
    "perlin": ("perlin", 48, "std16x9", "perlin", 2.0, 8),
    "cornell": ("cornell", 40, "square", "cornell", 300.0, 8),
    "final:6:60": ("final", 40, "square", "final:6:60", 0.0, 8),
}
LIT = ("cornell", "random-night")   # the scenes that list a light
BOOK2 = ("final:6:60",)


class Plan:
    """How a scene is uploaded: the upload-time switches (SHIRLEY_<key>) and the node placement flag.  `last`: the
    value of SHIRLEY_LDS_NODES is the scene's n_nodes4 - 1."""

    def __init__(self, name, nodes="auto", last=False, **env):
        self.name, self.nodes, self.last, self.env = name, nodes, last, env

    def __repr__(self):
        return self.name


DEFAULT = Plan("default")
GLOBAL = Plan("global", nodes="global")
NATURAL = Plan("wide-tree-natural")
NO_PRIMS = Plan("wide-tree-forced", NO_LDS_PRIMS="1")
NO_PERLIN = Plan("scene-lds-perlin-global", NO_LDS_PERLIN="1")
NARROW_LDS = Plan("narrow-tree-lds", nodes="lds", NO_WIDE="1")
MIXED_1 = Plan("mixed-1", NO_WIDE="1", LDS_NODES="1")
MIXED_LAST = Plan("mixed-last", last=True, NO_WIDE="1")

# (scene, builder, the plan under test, the plan it is compared with).  gen_spheres side 4 gets the wide block with
# only its tree in LDS by itself, so its other plan is the tree in global memory (the 256-thread block).
# random-night is uploaded with the SAH builder: with the reference builder its primitives already stay out of LDS.
CASES = [
    ("spheres:4", "reference", NATURAL, GLOBAL), ("spheres:4", "sah", NATURAL, GLOBAL),
    ("random", "sah", NO_PRIMS, DEFAULT), ("cornell", "reference", NO_PRIMS, DEFAULT),
    ("random-night", "sah", NO_PRIMS, DEFAULT), ("perlin", "sah", NO_PRIMS, DEFAULT),
    ("perlin", "sah", NO_PERLIN, DEFAULT), ("final:6:60", "sah", NO_PERLIN, DEFAULT),
    ("random", "sah", NARROW_LDS, DEFAULT), ("cornell", "reference", NARROW_LDS, DEFAULT),
    ("final:6:60", "sah", NARROW_LDS, DEFAULT),
    ("random", "sah", MIXED_1, DEFAULT), ("random", "sah", MIXED_LAST, DEFAULT),
    ("final:6:60", "sah", MIXED_1, DEFAULT), ("final:6:60", "sah", MIXED_LAST, DEFAULT),
]
# The default plan of every (scene, builder) above, for the comparison with the oracle.
BASES = sorted({(s, b, other) for s, b, _, other in CASES} | {("spheres:4", b, NATURAL) for b in ("reference", "sah")},
               key=repr)

# Entry points by group.  The tile passes and rt_scene_occluded return RT_E_UNSUPPORTED for a scene with book-2
# objects (tests/test_gpu_features.py, test_gpu_ao.py, test_gpu_direct.py, test_gpu_nee.py and test_gpu_occlusion.py
# expect that error), so those groups are skipped there and the ray group leaves rt_scene_occluded out.
GROUPS = ("render", "adaptive", "rays", "tiles", "lights")


def group_params(rows):
    out = []
    for row in rows:
        scene = row[0]
        for g in GROUPS:
            marks = []
            if g == "lights" and scene not in LIT and scene not in BOOK2:
                continue  # (no listed light: nothing dispatches)
            if g in ("tiles", "lights") and scene in BOOK2:
                marks = [pytest.mark.skip(reason="the tile passes return RT_E_UNSUPPORTED for a book-2 scene")]
            out.append(pytest.param(*row, g, marks=marks, id="-".join(str(x) for x in row[:3]) + "-" + g))
    return out


# ---- scenes, cameras, oracles: built once ------------------------------------------------------------------
class Shared:
    """Per scene: the finalized scene, its camera and oracle (made on demand, once); per (scene, builder, plan,
    group): the device's results under that plan (likewise), left unchanged."""

    def __init__(self):
        self.scenes, self.results, self.oracle = {}, {}, {}

    def scene(self, name):
        if name not in self.scenes:
            cam_scene, width, aspect = SCENES[name][:3]
            sc = rt.SceneBuilder.builtin(name, SEED).finalize(SEED)
            self.scenes[name] = (sc, rt.scene_camera(cam_scene, width, aspect), O.OracleScene(sc))
        return self.scenes[name]

    def once(self, key, make):
        if key not in self.oracle:
            self.oracle[key] = make()
        return self.oracle[key]


@pytest.fixture(scope="module")
def shared():
    return Shared()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.fixture(autouse=True)
def default_plan_again(monkeypatch):
    """No switch is set when a test begins.  (The light pick and the sampling mode a test sets last until the next
    upload, which every test of the suite begins with.)"""
    for k in SWITCHES:
        monkeypatch.delenv("SHIRLEY_" + k, raising=False)


@contextlib.contextmanager
def switches(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv("SHIRLEY_" + k, v)
    try:
        yield
    finally:
        for k in env:
            monkeypatch.delenv("SHIRLEY_" + k, raising=False)


def fixture_case(scene, bvh, tuning=""):
    return f"{scene}/0x5EED/{bvh}/default" + (f"/{tuning}" if tuning else "")


def upload(gpu, monkeypatch, golden, sc, scene, bvh, plan):
    """Upload under `plan` (its switches are set for rt_scene_upload alone) and assert the premise: the plan the
    device now runs differs from the scene's default plan in the intended field.

    tests/test_scene_plan.py pins tests/golden/scene_plan.json to compile_scene, and its
    test_scene_compile_reads_the_environment_in_one_place pins that an upload reads the same variables; the
    digest ties the uploaded scene and builder to the fixture's case.  Where the fixture holds the case under the
    switch, the field is read there.  Where it does not, the lines of csrc/rt/scene_compile.cpp (plan_placement)
    that decide it are named, from the fixture's default plan of the scene, and rt_scene_stats.wide_block — all the
    ABI shows of a placement — is asserted."""
    env = dict(plan.env)
    dflt = golden[fixture_case(scene, bvh)]
    if plan.last:
        env["LDS_NODES"] = str(dflt["n_nodes4"] - 1)
    with switches(monkeypatch, env):
        gpu.upload(sc, bvh, plan.nodes)
    st = gpu.stats()
    assert f"{gpu.digest():016x}" == dflt["digest"]
    assert dflt["wide"] == 1 and dflt["n_lds_nodes4"] == dflt["n_nodes4"] == st.n_nodes4  # every default here: wide
    tuning = ",".join(f"{k}={v}" for k, v in plan.env.items())
    var = golden.get(fixture_case(scene, bvh, tuning)) if tuning and plan.nodes == "auto" and not plan.last else None
    if plan is DEFAULT:
        assert st.wide_block == 1
    elif plan is NATURAL:
        # the wide block with the tree alone, by itself (the fixture's spheres:4 cases; test_the_flips_are_flips)
        assert (dflt["wide"], dflt["n_lds_prims"], dflt["n_lds_mats"]) == (1, 0, 0) and st.wide_block == 1
    elif plan is GLOBAL:
        # RT_BVH_NODES_GLOBAL: `placement == 0 || placement == RT_BVH_NODES_LDS` fails, so P.wide = false, and
        # lds_count returns 0 (its last line): the 256-thread block, kNodesGlobal (fixture: spheres:11/*/global)
        assert st.wide_block == 0
    elif plan is NO_PRIMS:
        # prims_lds = P.wide && ... && !tune.no_lds_prims -> n_lds_prims = n_lds_mats = n_lds_texs = 0, while P.wide
        # does not read the switch: (Wide, kNodesLds)
        assert dflt["n_lds_prims"] == dflt["n_objects"] > 0
        if var is not None:  # random/sah
            assert (var["wide"], var["n_lds_nodes4"], var["n_lds_prims"], var["n_lds_mats"]) == (1, dflt["n_nodes4"], 0, 0)
        assert st.wide_block == 1
    elif plan is NO_PERLIN:
        # perlin_lds = prims_lds && ... && !tune.no_lds_perlin -> n_lds_perlin = 0 with the primitives still in LDS:
        # kSceneLds with L.perlin == nullptr, wave_marble reads S.perlin
        assert dflt["n_lds_prims"] > 0 and dflt["n_lds_perlin"] == dflt["n_perlin"] > 0
        if var is not None:  # perlin/sah
            assert (var["wide"], var["n_lds_prims"], var["n_lds_perlin"]) == (1, dflt["n_lds_prims"], 0)
        assert st.wide_block == 1
    elif plan is NARROW_LDS:
        # P.wide = ... && !tune.no_wide -> false; n_lds_nodes4 = lds_count(stack4_bytes, ...) = `room` under
        # RT_BVH_NODES_LDS, and the tree that fits beside the wide block's 1024 (768) stacks (dflt["wide"]) fits beside
        # the 256-thread block's: room = n_nodes4, node_mode4 = kNodesLds.  The collapse does not read the switch.
        assert st.wide_block == 0
    else:
        # as above with placement 0: lds_count returns min(room, SHIRLEY_LDS_NODES) = k, 0 < k < n_nodes4: kNodesMixed
        # (fixture: spheres:11/sah/default/LDS_NODES=100)
        assert 0 < int(env["LDS_NODES"]) < dflt["n_nodes4"] and st.wide_block == 0
    return st


# ---- the entry points ----------------------------------------------------------------------------------------
def settings(**kw):
    return rt.RenderSettings(**{**dict(samples=SPP, max_reflect=DEPTH, seed=SEED, sample_chunk=SPP,
                                       engine="megakernel"), **kw})


def rays_of(shared, scene):
    def make():
        sc, cam, _ = shared.scene(scene)
        rays = random_scene_rays(N_RAYS) if scene in ("random", "random-night") else scene_box_rays(sc, cam, N_RAYS)
        rng = np.random.default_rng(11)
        reach = 1000.0 if scene == "cornell" else 20.0
        return rays, np.exp(rng.uniform(np.log(0.05), np.log(reach), N_RAYS))
    return shared.once(("rays", scene), make)


def records(recs):
    for r in recs:
        if hasattr(r, "pad"):
            r.pad = 0
    return b"".join(bytes(r) for r in recs)


def run_group(gpu, shared, scene, group):
    """The group's entry points on the scene now uploaded -> {name: arrays / bytes / tuples}."""
    sc, cam, _ = shared.scene(scene)
    spp = SCENES[scene][5]
    out = {}
    if group == "render":
        out["frame"] = gpu.render(cam, settings(samples=spp, sample_chunk=spp))
        c = gpu.counters()
        out["counters"] = (int(c.samples), int(c.segments))
        assert c.engine == 1 and c.samples == cam.image_width * cam.image_height * spp
    elif group == "adaptive":
        # threshold 0: every tile goes through both steps' tile lists (the LIST instance), one-sample batches
        s = settings(samples=spp, sample_chunk=1)
        accum, counts, moments, tile_error, rep = gpu.render_adaptive(
            cam, s, rt.AdaptiveSettings(threshold=0.0, min_samples=spp // 2, step=spp // 2, noise_floor=0.01))
        assert (counts == spp).all() and rep.steps == 2 and rep.samples == counts.sum()
        out.update(accum=accum, counts=counts, moments=moments, tile_error=tile_error,
                   report=(int(rep.samples), int(rep.segments), int(rep.steps)))
        out["uniform"] = gpu.render(cam, s)
    elif group == "rays":
        rays, t_each = rays_of(shared, scene)
        out["render"] = gpu.hit(rays, 0.001, float("inf"), traversal="render")
        out["binary"] = gpu.hit(rays, 0.001, float("inf"), traversal="binary")
        out["probe"] = gpu.probe(rays, SEED)
        if scene not in BOOK2:
            out["occluded"] = gpu.occluded(rays, 0.001, t_each)
    elif group == "tiles":
        radius = SCENES[scene][4]
        s = rt.RenderSettings(samples=SPP, seed=SEED)
        out["features0"] = gpu.render_features(cam, s, chain=0)
        out["features8"] = gpu.render_features(cam, s, chain=8)
        out["ao"] = gpu.render_ao(cam, s, chain=8, radius=radius)
    elif group == "lights":
        s = rt.RenderSettings(samples=SPP, max_reflect=DEPTH, seed=SEED)
        out["direct"] = gpu.render_direct(cam, s, chain=8)
        out["nee"] = gpu.render_nee(cam, s, mis=False)
        out["nee_mis"] = gpu.render_nee(cam, s, mis=True)
        info = gpu.light_pick(4)
        gpu.light_sampling(N.RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL)
        out["grid"] = (tuple(info.n), int(info.n_lights))
        out["pick_direct"] = gpu.render_direct(cam, s, chain=8)
        out["pick_nee_mis"] = gpu.render_nee(cam, s, mis=True)
        rep = gpu.light_visibility(4, SEED)
        out["masks"] = gpu.light_visibility_masks()
        out["visibility"] = (int(rep.pairs), int(rep.traced), int(rep.unoccluded), int(rep.dead_points))
        out["vis_direct"] = gpu.render_direct(cam, s, chain=8)
        out["vis_nee_mis"] = gpu.render_nee(cam, s, mis=True)
    return out


def same(a, b):
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, (list, tuple)) and a and isinstance(a[0], np.ndarray):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, list):
        return records(a) == records(b)
    return a == b


def results(gpu, monkeypatch, golden, shared, scene, bvh, plan, group):
    key = (scene, bvh, plan.name, group)
    if key not in shared.results:
        upload(gpu, monkeypatch, golden, shared.scene(scene)[0], scene, bvh, plan)
        shared.results[key] = run_group(gpu, shared, scene, group)
    return shared.results[key]


# ---- a placement changes no bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,bvh,plan,other,group", group_params(CASES))
def test_placement_changes_no_bit(gpu, monkeypatch, golden, shared, scene, bvh, plan, other, group):
    want = results(gpu, monkeypatch, golden, shared, scene, bvh, other, group)
    upload(gpu, monkeypatch, golden, shared.scene(scene)[0], scene, bvh, plan)
    got = run_group(gpu, shared, scene, group)
    assert sorted(got) == sorted(want)
    for name in want:
        assert same(got[name], want[name]), f"{scene}/{bvh} {plan} against {other}: {name} differs"
    if group == "rays":
        # the render traversal against the 2-wide f64 one, record for record, under the plan itself
        n_hit = 0
        for a, b in zip(got["render"], got["binary"]):
            assert a.object == b.object and (a.object < 0 or (_same_record(a, b) and a.u == b.u and a.v == b.v))
            n_hit += a.object >= 0
        assert n_hit > 200


# ---- the plan compared with: the oracle's --------------------------------------------------------------------
@pytest.mark.parametrize("scene,bvh,plan,group", group_params(BASES))
def test_compared_plan_matches_the_oracle(gpu, monkeypatch, golden, shared, scene, bvh, plan, group):
    got = results(gpu, monkeypatch, golden, shared, scene, bvh, plan, group)
    sc, cam, osc = shared.scene(scene)
    floor, spp = exact_floor(SCENES[scene][3]), SCENES[scene][5]
    if group == "render":
        ora, ocnt = shared.once(("render", scene), lambda: osc.render(cam, O.params(spp, DEPTH, SEED), threads=16))
        check_parity(got["frame"], ora, spp, frac_exact=floor)
        assert got["counters"][0] == ocnt.samples
        assert abs(got["counters"][1] - int(ocnt.segments)) <= 0.001 * ocnt.segments
    elif group == "adaptive":
        # the list path's frame is the uniform frame of one-sample units, and that the oracle's in-order frame
        ora, _ = shared.once(("render", scene), lambda: osc.render(cam, O.params(spp, DEPTH, SEED), threads=16))
        assert np.array_equal(got["accum"], got["uniform"])
        check_parity(got["uniform"], ora, spp, frac_exact=floor)
    elif group == "rays":
        rays, t_each = rays_of(shared, scene)
        if scene in BOOK2:
            # media draw their free flight through log (ocml against glibc): the closest object, as
            # test_hit_queries_book2_match_oracle compares it
            n_hit = 0
            for i, g in enumerate(got["render"]):
                h = osc.hit(rays[i], 0.001, float("inf"), index=i)
                assert g.object == (h.object if h.hit else -1), i
                n_hit += bool(h.hit)
            assert n_hit > 200
        else:
            _check_against_oracle(got["render"], rays, osc, 200)
            want = shared.once(("occluded", scene), lambda: oracle_occluded(osc, rays, t_each))
            assert 0.05 <= want.mean() <= 0.95 and np.array_equal(got["occluded"], want)
        # the probe's record is the closest hit's (a medium's free flight is drawn on the probe's own path key, so
        # on the book-2 scene the closest object is the oracle's probe's, on that key)
        for i, (p, h) in enumerate(zip(got["probe"], got["render"])):
            if scene in BOOK2:
                assert p.object == osc.probe(rays[i], SEED, i).object, i
            else:
                assert p.object == h.object and (p.object < 0 or (p.t == h.t and list(p.normal) == list(h.normal)))
    elif group == "tiles":
        for chain in (0, 8):
            want = shared.once(("features", scene, chain), lambda: oracle_features(sc, cam, SEED, 0, SPP, chain))
            check_features(got[f"features{chain}"], want, SPP, f"{scene} {plan} chain {chain}")
        ref = shared.once(("ao", scene), lambda: ao_ref.oracle_ao(sc, cam, SEED, 0, SPP, 8, SCENES[scene][4], osc))
        assert np.array_equal(got["ao"], ref.sums), f"{int(np.sum(got['ao'] != ref.sums))} pixels differ"
        assert ref.vertices > 0 and 0 < ref.occluded < ref.vertices
    elif group == "lights":
        # the rules of tests/test_gpu_direct.py and tests/test_gpu_nee.py: exact where every vertex of the pixel has a
        # solid albedo; elsewhere (marble, checker: sin and floor) 1e-12 relative for the one-vertex estimate and the
        # parity rule's 1e-10 * spp on all but 0.1 % of the pixels for the path integrator
        dref = shared.once(("direct", scene), lambda: D.oracle_direct(sc, cam, SEED, 0, SPP, 8, osc))
        em, di = got["direct"]
        assert dref.sampled > 0 and dref.occluded > 0 and dref.unoccluded > 0
        assert np.array_equal(em[dref.solid], dref.emission[dref.solid])
        assert np.array_equal(di[dref.solid], dref.direct[dref.solid])
        for g, w in ((em, dref.emission), (di, dref.direct)):
            assert np.all(np.abs(g - w) <= 1e-12 * np.abs(w))
        for mis, name in ((False, "nee"), (True, "nee_mis")):
            ref = shared.once((name, scene), lambda: R.oracle_nee(sc, cam, SEED, 0, SPP, DEPTH, mis, osc, stats=False))
            bad = np.any(np.abs(got[name] - ref.sums) > 1e-10 * SPP, axis=-1)
            assert np.array_equal(got[name][ref.solid], ref.sums[ref.solid])
            assert bad.mean() <= 0.001
        # the masks of rt_scene_light_visibility, 4 cells, K = 4
        lights, _ = D.list_lights(sc.desc)
        masks = shared.once(("masks", scene), lambda: V.Masks(G.Grid(lights, 4), lights, osc, 4, SEED))
        assert got["grid"][1] == len(lights) and got["masks"].size == masks.masks.size
        assert np.array_equal(got["masks"].reshape(masks.masks.shape), masks.masks)
        assert got["visibility"] == (masks.masks.size, masks.traced, masks.unoccluded, masks.dead_points)
        # both passes under the 4-cell pick with solid-angle sampling of every light, on the grid's own rows and on
        # the visibility rows of those masks: the restatement of tests/test_gpu_light_rect.py and its criterion
        ALL = N.RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL
        grid = G.Grid(lights, 4)
        vis = V.grid_with(grid, V.rows(grid, lights, masks.masks, 4))
        for prefix, rows in (("pick", None), ("vis", vis)):
            def restate(f, *a):
                with V.visibility_rows(rows) if rows is not None else contextlib.nullcontext():
                    return f(sc, cam, SEED, 0, SPP, *a, 4, ALL, osc)
            dref = shared.once((prefix, "direct", scene), lambda: restate(RR.oracle_direct, 8))
            nref = shared.once((prefix, "nee", scene), lambda: restate(RR.oracle_nee, DEPTH, True))
            em, di = got[prefix + "_direct"]
            parity_where_solid(em, dref.emission, dref.solid, SPP)
            parity_where_solid(di, dref.direct, dref.solid, SPP)
            parity_where_solid(got[prefix + "_nee_mis"], nref.sums, nref.solid, SPP)
            assert dref.occluded > 0 and dref.unoccluded > 0 and nref.sums.max() > 0.0
