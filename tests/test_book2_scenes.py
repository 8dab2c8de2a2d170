"""The inputs of tests/test_gpu_book2.py (tests/book2_scenes.py) checked with the oracle alone, so that the device
tests' coverage holds by construction: every object form is the closest hit of rays of its scene, every medium
scatters and lets pass, both sides of DExt index 32 are met by the same rays, the oracle's tree agrees with the plain
list of objects, and the twin scenes' frames are equal on the oracle bit for bit."""
import ctypes as C

import numpy as np
import pytest

import book2_scenes as B
import oracle_lib as O
from raytracer import _native as N

NAMES = ["zoo", "zoo_solid", "smoke", "many_ext", "shutter"]
INF = float("inf")


def object_hit(o, ray, t_min=B.T_MIN, t_max=INF):
    h = O.or_hit()
    return h if O.lib().or_object_hit(C.byref(o), O.d6(ray), t_min, t_max, C.byref(h)) else None


def never_hit(name):
    return {B.SMOKE_BOUNDARY_RECT} if name == "smoke" else set()


@pytest.mark.parametrize("name", NAMES)
def test_every_object_is_the_closest_hit_of_rays(name):
    scene, _, sets = B.get(name)
    wins = np.zeros(scene.desc.n_objects, dtype=int)
    for s, rec in B.oracle_hits(name).items():
        assert len(rec) == len(sets[s][0])
        wins += np.bincount(rec["object"][rec["hit"] != 0], minlength=len(wins))
    for i, w in enumerate(wins):
        if i in never_hit(name):
            assert w == 0, f"object {i}: a rect as a medium boundary scattered"
        else:
            assert w >= 16, f"object {i} is the closest hit of {w} rays"


def test_scenes_hold_the_forms_the_device_tests_name():
    """What each scene must contain, read from the finalized descriptions."""
    geoms = [N.RT_GEOM_SPHERE, N.RT_GEOM_MOVING_SPHERE, N.RT_GEOM_RECT_XY, N.RT_GEOM_RECT_YZ, N.RT_GEOM_RECT_XZ,
             N.RT_GEOM_RECT_BOX]
    scene = B.get("zoo")[0]
    objs = B.objects(scene)
    for g in geoms:
        assert any(o.geometry == g and not o.transform for o in objs), g
        assert any(o.geometry == g and o.transform and o.rotate_y_deg != 0 and any(o.offset)
                   and B.is_extended(scene, i) for i, o in enumerate(objs)), g
    angles = {o.rotate_y_deg for o in objs if o.transform}
    assert min(angles) < 0 and max(angles) > 90 and len(angles) >= 6
    assert sum(B.is_flattened(scene, i) for i in range(len(objs))) == 1
    assert not any(o.medium for o in objs)
    assert len(B.objects(B.get("zoo_solid")[0])) == len(objs) - 3
    media = [o for o in B.objects(B.get("smoke")[0]) if o.medium]
    forms = {(o.geometry, bool(o.transform)) for o in media}
    assert {(N.RT_GEOM_RECT_BOX, True), (N.RT_GEOM_SPHERE, False), (N.RT_GEOM_SPHERE, True),
            (N.RT_GEOM_MOVING_SPHERE, False), (N.RT_GEOM_RECT_XY, False)} <= forms
    assert sorted(o.rotate_y_deg for o in media if o.geometry == N.RT_GEOM_RECT_BOX) == [-18.0, 15.0]
    scene = B.get("many_ext")[0]
    ext = B.ext_index(scene)
    assert len(ext) >= 48 and sorted(ext.values()) == list(range(len(ext)))
    kinds = {(o.geometry, bool(o.medium)) for i, o in enumerate(B.objects(scene)) if i in ext}
    assert len(kinds) >= 7
    spans = {(o.q[3], o.q[4]) for o in B.objects(B.get("shutter")[0]) if o.geometry == N.RT_GEOM_MOVING_SPHERE}
    assert spans == {(0.0, 1.0), (-1.0, 3.0)}


def medium_exit(o, ray, t_max):
    """Where a ray leaves a medium's boundary for the last time before t_max, or None if it never meets the
    boundary: the hits of the medium's shape taken as a surface."""
    surface = type(o).from_buffer_copy(o)
    surface.medium = 0
    t, last = B.T_MIN, None
    for _ in range(4):
        h = object_hit(surface, ray, t, t_max)
        if h is None:
            break
        last = h.t
        t = h.t + 1e-4
    return last


def test_smoke_media_scatter_and_let_pass():
    scene, _, sets = B.get("smoke")
    objs = B.objects(scene)
    hits = B.oracle_hits("smoke")
    for i, o in enumerate(objs):
        if not o.medium or i == B.SMOKE_BOUNDARY_RECT:
            continue
        scatters = passes = inside = 0
        for s, (rays, t_max) in sets.items():
            rec = hits[s]
            inside += int(B.contains(o, rays[:, :3]).sum())
            scatters += int(((rec["hit"] != 0) & (rec["object"] == i)).sum())
            for k in np.nonzero((rec["hit"] == 0) | (rec["object"] != i))[0]:
                # passed: the ray left the medium before its closest hit (or before t_max, if it hit nothing)
                end = rec["t"][k] if rec["hit"][k] else t_max
                if medium_exit(o, rays[k], end) is not None and medium_exit(o, rays[k], INF) == medium_exit(o, rays[k], end):
                    passes += 1
        assert scatters >= 50 and passes >= 50 and inside >= 16, (i, scatters, passes, inside)


def test_many_ext_meets_both_sides_of_index_32():
    """Objects with a DExt index below 32 are deferred to the end of a traversal, the others are tested inside its
    loop (rt_device.h leaf_tests4).  A ray `crosses` an object's box when the box passes the reference's slab test
    on [t_min, the ray's closest hit]: no traversal can cull such a box, so the object's own test runs."""
    scene, _, sets = B.get("many_ext")
    ext = B.ext_index(scene)
    objs = B.objects(scene)
    boxes = {i: O.d6(B.bbox(objs[i])) for i in ext}
    wins = {True: 0, False: 0}
    both = 0
    for s, rec in B.oracle_hits("many_ext").items():
        rays, t_max = sets[s]
        for k in range(len(rays)):
            if rec["hit"][k] and int(rec["object"][k]) in ext:
                wins[ext[int(rec["object"][k])] < 32] += 1
            end = rec["t"][k] if rec["hit"][k] else t_max
            r = O.d6(rays[k])
            met = {ext[i] < 32 for i, b in boxes.items() if O.lib().or_aabb_hit2(b, r, B.T_MIN, end)}
            both += len(met) == 2
    assert wins[True] >= 100 and wins[False] >= 100 and both >= 100, (wins, both)


@pytest.mark.parametrize("name", NAMES)
def test_tree_agrees_with_the_list(name):
    """A closest hit on a non-medium object is the minimum of or_object_hit over the non-medium objects, record for
    record; a flattened sphere's within rounding (the scene holds the flattened sphere, the list the instance).  A
    medium's scatter, or a miss, lies in front of every surface.  (A medium's own test draws from a stream keyed
    by the object and the ray, which or_object_hit has not: the list is of surfaces.)"""
    scene, _, sets = B.get(name)
    objs = B.objects(scene)
    surfaces = [i for i, o in enumerate(objs) if not o.medium]
    checked = 0
    for s, rec in B.oracle_hits(name).items():
        rays, t_max = sets[s]
        for k in range(len(rays)):
            best, who = None, -1
            for i in surfaces:
                h = object_hit(objs[i], rays[k], B.T_MIN, t_max)
                if h is not None and (best is None or h.t < best.t):
                    best, who = h, i
            if rec["hit"][k] and not objs[rec["object"][k]].medium:
                assert who == rec["object"][k], (s, k)
                if B.is_flattened(scene, who):
                    assert abs(best.t - rec["t"][k]) <= 1e-12 * best.t
                    assert np.allclose(list(best.point), rec["point"][k], rtol=1e-12, atol=1e-12)
                    assert abs(best.u - rec["u"][k]) < 1e-12 and abs(best.v - rec["v"][k]) < 1e-12
                else:
                    assert (best.t, list(best.point), list(best.normal), best.front_face, best.u, best.v) == \
                        (rec["t"][k], list(rec["point"][k]), list(rec["normal"][k]), rec["front_face"][k], rec["u"][k],
                         rec["v"][k]), (s, k)
                checked += 1
            elif rec["hit"][k]:
                assert best is None or best.t >= rec["t"][k], (s, k)
            else:
                assert best is None, (s, k)
    assert checked >= 1000


def oracle_frame(scene, cam, spp=4, depth=16):
    img, cnt = O.OracleScene(scene).render(cam, O.params(spp, depth, B.SEED), threads=8)
    return img, (int(cnt.samples), int(cnt.segments))


@pytest.mark.parametrize("key", B.TWINS)
def test_twins_are_equal_on_the_oracle(key):
    ext, bare, cam = B.twin(key)
    a, ca = oracle_frame(ext, cam)
    b, cb = oracle_frame(bare, cam)
    assert np.array_equal(a, b) and ca == cb
    assert np.isfinite(a).all() and np.mean(a > 0) > 0.9 and len(np.unique(a)) > 30


def test_open_shutter_differs_from_both_frozen_ends():
    frames = {w: oracle_frame(*B.shutter(w)[:2])[0] for w in ("open", "inner", "frozen", "frozen0", "frozen1")}
    for w in ("inner", "frozen", "frozen0", "frozen1"):
        assert np.mean(frames["open"] != frames[w]) > 0.02, w
    assert np.mean(frames["frozen0"] != frames["frozen1"]) > 0.02
