"""Exact ties in t: two primitives hit at the same binary64 t.

The reference accepts a hit at t == the running closest t (sphere.rs:40-45 rejects only `t_max < root`,
rect.rs:58 only `t > t_max`), so the tied primitive tested LAST wins — provided its bounding box passes
`hit2` (aabb.rs:62-79), whose `t_max <= t_min` test is strict, at t_max = the tie.  bbox_tree.rs:56-91
pops rhs before lhs, so the last one tested is the leftmost leaf of the reference tree whose box passes.
The device numbers its primitives in that leaf order (scene_compile.cpp reference_ranks) and compares two tested
candidates at an equal t by it (rt_device.h tie_takes); a traversal that skipped a box failing at the
closest t by no more than rounding re-decides the winner once at its end from all tied primitives
(resolve_ties; the rule is pinned on CPU in test_tie_rule.py) — whatever tree it traverses (SAH by
default) and in whatever order.
No reference scene produces a tie (the random scene's coat, y in [-0.01, 0], lies 0.01 above its lower
surface at y = -0.02: scenes.rs:251-279; the Cornell walls meet only at edges).  Constructed here: two
coincident spheres, and an xz_rect coplanar with a RectBox's top face.  The tests assert the reference's
(the oracle's) choice ray by ray on both traversals, and frames within the parity tolerance."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import raytracer as rt
from raytracer import _native as N
from test_scatter_kat import KatScene

pytestmark = pytest.mark.gpu
SEED = 0x5EED
RED = {"kind": N.RT_TEX_SOLID, "color": (0.9, 0.1, 0.1)}
GREEN = {"kind": N.RT_TEX_SOLID, "color": (0.1, 0.9, 0.1)}
MATS = [(N.RT_MAT_LAMBERTIAN, 0, (0, 0, 0), 0.0), (N.RT_MAT_LAMBERTIAN, 1, (0, 0, 0), 0.0)]


def _root_children(scene):
    """(lhs leaf object, rhs leaf object) of the reference builder's root (the tree both sides build)."""
    n = C.c_int32(0)
    assert N.rt_lib().rt_bvh_build_host(scene.desc_ptr, N.RT_BVH_REFERENCE, C.byref(n), None, None) == 0
    arr = (N.rt_bvh_node * n.value)()
    root = C.c_int32(0)
    assert N.rt_lib().rt_bvh_build_host(scene.desc_ptr, N.RT_BVH_REFERENCE, C.byref(n), arr, C.byref(root)) == 0
    r = arr[root.value]
    return arr[r.lhs].leaf, arr[r.rhs].leaf


def _log(name, **kv):
    path = os.environ.get("SHIRLEY_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": name, **kv}) + "\n")


def _frame_departure(gpu, scene, cam, spp=4):
    img = gpu.render(cam, rt.RenderSettings(samples=spp, seed=SEED, sample_chunk=spp))
    ora, _ = O.OracleScene(scene.desc).render(cam, O.params(spp, 50, SEED))
    bad = np.any(np.abs(img - ora) > 1e-10 * spp, axis=-1)
    return float(bad.mean()), float(np.mean(img == ora))


def _upload(gpu, scene, bvh):
    rt.Device.upload(gpu, type("S", (), {"desc_ptr": scene.desc_ptr})(), bvh=bvh)


@pytest.mark.parametrize("bvh", ["reference", "sah"])
def test_coincident_spheres_tie(gpu, bvh):
    scene = KatScene([(N.RT_GEOM_SPHERE, 0, [0.0, 0.0, -3.0, 1.0]), (N.RT_GEOM_SPHERE, 1, [0.0, 0.0, -3.0, 1.0])],
                     MATS, [RED, GREEN])
    lhs, rhs = _root_children(scene)
    assert {lhs, rhs} == {0, 1}
    _upload(gpu, scene, bvh)
    osc = O.OracleScene(scene.desc)
    rng = np.random.default_rng(11)
    # rays from around (0, 0, 2) at the sphere, off the axes (the hit point strictly inside the box's faces)
    tgt = np.array([0.0, 0.0, -3.0]) + rng.uniform(-0.5, 0.5, size=(256, 3))
    org = np.array([0.3, 0.2, 2.0]) + rng.uniform(-0.5, 0.5, size=(256, 3))
    rays = np.hstack([org, tgt - org])
    for traversal in ("render", "binary"):
        dev = gpu.hit(rays, 0.001, float("inf"), traversal=traversal)
        for i, ray in enumerate(rays):
            h = osc.hit(ray)
            g = dev[i]
            assert h.hit and h.object == lhs   # the reference: lhs tested last
            assert g.object == lhs, (traversal, i)
            assert (g.t, list(g.point), list(g.normal), g.front_face) == (h.t, list(h.point), list(h.normal),
                                                                           h.front_face)
    # the frame: the sphere shows the other material wherever it is seen first-hand
    cam = rt.CameraBuilder(width=32, aspect_ratio=(1, 1), vfov=40.0).build(rt.CameraPosition((0.0, 0.0, 2.0),
                                                                                             (0.0, 0.0, -3.0)))
    dep, exact = _frame_departure(gpu, scene, cam)
    _log("ties:coincident_spheres", departure_px=dep, exact=exact)
    assert dep <= 0.001 and exact >= 0.99  # the parity tolerance (round 5, first-tested wins: 26 % departed)


@pytest.mark.parametrize("bvh", ["reference", "sah"])
def test_rect_coplanar_with_rectbox_face_tie(gpu, bvh):
    # RectBox [-1, 1] x [-1, 0] x [-4, -2] and xz_rect [-1, 1] x [-4, -2] at y = 0: its top face, exactly
    for order in ("box_first", "rect_first"):
        box = (N.RT_GEOM_RECT_BOX, 0, [-1.0, -1.0, -4.0, 1.0, 0.0, -2.0])
        rect = (N.RT_GEOM_RECT_XZ, 1, [-1.0, 1.0, -4.0, -2.0, 0.0])
        objs = [box, rect] if order == "box_first" else [rect, box]
        mats = MATS if order == "box_first" else MATS
        scene = KatScene(objs, mats, [RED, GREEN])
        rect_id = 1 if order == "box_first" else 0
        _upload(gpu, scene, bvh)
        osc = O.OracleScene(scene.desc)
        rng = np.random.default_rng(12)
        tgt = np.column_stack([rng.uniform(-0.9, 0.9, 256), np.zeros(256), rng.uniform(-3.9, -2.1, 256)])
        org = tgt + np.column_stack([rng.uniform(-1, 1, 256), rng.uniform(0.5, 3, 256), rng.uniform(-1, 1, 256)])
        # 32 vertical rays of direction (0, -1, 0): 1/d is exact, so the box's slab entry at y = 0 IS the tie
        org[:32] = tgt[:32] + np.array([0.0, 1.0, 0.0])
        rays = np.hstack([org, tgt - org])
        n_ref_rect = 0
        for traversal in ("render", "binary"):
            dev = gpu.hit(rays, 0.001, float("inf"), traversal=traversal)
            n_ref_rect = 0
            for i, ray in enumerate(rays):
                h = osc.hit(ray)
                g = dev[i]
                assert h.hit and g.object == h.object, (order, traversal, i, g.object, h.object)
                assert (g.t, list(g.point), list(g.normal)) == (h.t, list(h.point), list(h.normal))
                n_ref_rect += h.object == rect_id
                if i < 32:
                    # vertical rays: the box's slab entry at y = 0 is exactly the tie, and hit2's strict
                    # `t_max <= t_min` rejects the box whichever is tested last: the rect wins
                    assert h.object == rect_id
            assert 32 <= n_ref_rect < len(rays) or order == "rect_first"
        _log(f"ties:rect_on_rectbox_face:{order}", reference_rect_fraction=n_ref_rect / len(rays))
        cam = rt.CameraBuilder(width=32, aspect_ratio=(1, 1), vfov=40.0).build(
            rt.CameraPosition((0.0, 3.0, 0.5), (0.0, 0.0, -3.0)))
        dep, exact = _frame_departure(gpu, scene, cam)
        _log(f"ties:rect_on_rectbox_face_frame:{order}", departure_px=dep, exact=exact)
        assert dep <= 0.001 and exact >= 0.99  # (round 5: 11.7 % departed with the box first)


@pytest.mark.parametrize("bvh", ["reference", "sah"])
def test_every_hit_a_tie_matches_the_reference(gpu, bvh):
    """random_scene with every object twice — the copy right after the original, with a red Lambertian
    instead of the original material — so that every hit of every path is an exact tie between two
    primitives, and the winner decides the colour and the path.  The frame must follow the reference's
    choice (the oracle walks the reference tree rhs-first, bbox_tree.rs:76-80) on both trees the device
    can walk; round 5's device chose by its own test order here."""
    from test_gpu_parity import check_parity
    src = json.loads(rt.scenes.random_scene(SEED).to_json())
    red = {"Lambertian": {"albedo": {"Solid": {"vec": [0.9, 0.1, 0.05]}}}}
    objs = []
    for o in src["objects"]:
        objs.append(o)
        objs.append({**o, "material": red})
    src["objects"] = objs
    scene = rt.SceneBuilder.from_json(json.dumps(src)).finalize(SEED)
    gpu.upload(scene, bvh)
    # the query agrees ray by ray, object index included (the tied pair differ only in material)
    rng = np.random.default_rng(3)
    rays = np.hstack([np.array([13.0, 2.0, 3.0]) + rng.normal(scale=0.2, size=(512, 3)),
                      rng.uniform([-13.0, -2.5, -3.5], [-9.0, -1.5, 1.5], size=(512, 3))])
    osc = O.OracleScene(scene)
    ref = [osc.hit(r) for r in rays]
    for traversal in ("render", "binary"):
        bad = [(i, g.object, h.object, h.t) for i, (g, h) in enumerate(zip(gpu.hit(rays, 0.001, float("inf"),
                                                                               traversal=traversal), ref))
               if g.object != (h.object if h.hit else -1)]
        _log(f"ties:duplicated_random_scene_rays:{bvh}:{traversal}", bad=len(bad), first=bad[:8],
             rays=rays[[b[0] for b in bad[:8]]].tolist())
        assert not bad, (traversal, len(bad), bad[:4])
    assert sum(h.hit for h in ref) > 100
    cam = rt.default_camera(48, "std16x9")
    spp = 4
    for depth in (1, 2, 3):  # (diagnostic: the bounce at which a departure starts)
        i_d = gpu.render(cam, rt.RenderSettings(samples=spp, max_reflect=depth, seed=SEED, sample_chunk=spp))
        o_d, _ = O.OracleScene(scene).render(cam, O.params(spp, depth, SEED))
        _log(f"ties:duplicated_random_scene_depth:{bvh}:{depth}",
             departure_px=float(np.any(np.abs(i_d - o_d) > 1e-10 * spp, axis=-1).mean()))
    img = gpu.render(cam, rt.RenderSettings(samples=spp, max_reflect=50, seed=SEED, sample_chunk=spp))
    ora, _ = O.OracleScene(scene).render(cam, O.params(spp, 50, SEED))
    dep = float(np.any(np.abs(img - ora) > 1e-10 * spp, axis=-1).mean())
    _log(f"ties:duplicated_random_scene:{bvh}", departure_px=dep, exact=float(np.mean(img == ora)))
    check_parity(img, ora, spp)
