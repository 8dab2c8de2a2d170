"""Synthetic ground stacks for the hop pass (scene_compile.cpp ground_stack, rt_device.h ground_hop):
a family of small scenes, one per premise of the proof the pass rests on, and two 32x32 cameras per scene that
put most of the frame's first hits on the coat.  A plain helper (tests/test_ground_hop.py on the CPU,
tests/test_gpu_hop_scenes.py on the device).

Every coordinate is a binary fraction, so the record's comparisons (a sphere's box starting at or above the top
plane, planes a gap apart) hold or fail exactly as written here, and the JSON round trip is exact.

  slab(Y)   a grey ground rect at Y - h - sep and, over it, a glass coat (RectBox, ir 1.5) of thickness h whose top
            is Y: random_scene's ground, flat and 8 x 8
  balls(Y)  six spheres resting on Y (radii 1/8, 3/16, 1/4; Lambertian, metal, glass), in two rows

KIND names the hop pass scene compilation must choose (rt_scene_stats.hop_kind): 2 the ground stack's, 1 the
first-node visit.  RECORD holds (n, n_box, y_top, guarded) of the kind-2 scenes' DGround records."""
import json

import raytracer as rt

SEED = 0x5EED
H = 2.0 ** -7
SEP = 2.0 ** -10
GREY = {"Lambertian": {"albedo": {"Solid": {"vec": [0.5, 0.5, 0.5]}}}}


def vec(x, y, z):
    return {"vec": [float(x), float(y), float(z)]}


def lambertian(r, g, b):
    return {"Lambertian": {"albedo": {"Solid": vec(r, g, b)}}}


def metal(r, g, b, fuzz):
    return {"Metal": {"albedo": vec(r, g, b), "fuzz": float(fuzz)}}


def glass(ir):
    return {"Dielectric": {"ir": float(ir)}}


def rect_xz(x0, x1, z0, z1, y, material):
    return {"geometry": {"RectXZ": {"d1_min": float(x0), "d1_max": float(x1), "d2_min": float(z0), "d2_max": float(z1),
                                    "offset": float(y)}}, "material": material}


def rect_yz(y0, y1, z0, z1, x, material):
    return {"geometry": {"RectYZ": {"d1_min": float(y0), "d1_max": float(y1), "d2_min": float(z0), "d2_max": float(z1),
                                    "offset": float(x)}}, "material": material}


def box(lo, hi, material):
    # (from_json reads min and max alone: RectBox::new derives the sides)
    return {"geometry": {"RectBox": {"min": vec(*lo), "max": vec(*hi)}}, "material": material}


def sphere(c, r, material):
    return {"geometry": {"Sphere": {"center": vec(*c), "radius": float(r)}}, "material": material}


def ground_rect(y, ext=4.0, material=GREY):
    return rect_xz(-ext, ext, -ext, ext, y, material)


def coat(y0, y1, ir=1.5, ext=4.0):
    return box((-ext, y0, -ext), (ext, y1, ext), glass(ir))


def slab(y, sep=SEP, coat_ext=4.0):
    return [ground_rect(y - H - sep), coat(y - H, y, ext=coat_ext)]


BALL_MATERIALS = [lambertian(0.7, 0.2, 0.2), metal(0.8, 0.8, 0.6, 0.1), glass(1.5), lambertian(0.2, 0.6, 0.3),
                  metal(0.6, 0.6, 0.9, 0.0), glass(1.5)]


def ball_radius(i):
    return 0.125 + 0.0625 * (i % 3)


def ball_xz(i):
    return -1.5 + 0.75 * i, (-0.5 if i % 2 == 0 else 0.5)


def balls(y, lift=0.0):
    out = []
    for i in range(6):
        x, z = ball_xz(i)
        out.append(sphere((x, y + ball_radius(i) + lift, z), ball_radius(i), BALL_MATERIALS[i]))
    return out


def _two_coats():
    return [ground_rect(-0.0625 - SEP), coat(-0.0625, -0.03125, ir=1.3), coat(-0.015625, 0.0, ir=1.5),
            ground_rect(-0.0234375, material=lambertian(0.9, 0.9, 0.2))] + balls(0.0)


def _sunk():
    objs = slab(0.0) + balls(0.0)
    objs[-1]["geometry"]["Sphere"]["center"]["vec"][1] -= 2.0 ** -10
    return objs


def objects(name):
    """The object list of scene `name`; the order is part of the scene (the reference builds its tree from it, and
    the tree's leaf order decides an exact tie: DESIGN.md §8)."""
    slab0 = slab(0.0) + balls(0.0)
    table = {
        "slab0": lambda: slab0,
        "slab_up": lambda: slab(3.0) + balls(3.0),
        "slab_down": lambda: slab(-2.5) + balls(-2.5),
        "floating": lambda: slab(0.0) + balls(0.0, lift=0.25),  # above the guard's reach: no bitmap
        "bare": lambda: slab(0.0),  # no sphere at all
        "neg_radius": lambda: slab0 + [sphere((0.3, 0.1, 1.5), -0.1, GREY)],  # never hit (sphere_never_hit)
        "two_coats": _two_coats,  # two glass boxes of different ir, a rect between them
        "small_coat": lambda: slab(0.0, coat_ext=2.0) + balls(0.0),  # the coat ends inside the rect
        # the top plane is the raised rect's padded box (0.5 + 1e-4), not the coat's top
        "rect_top": lambda: [coat(-H, 0.0), ground_rect(-H - SEP), rect_xz(-1.5, -0.5, -0.5, 0.5, 0.5, lambertian(0.9, 0.1, 0.1))]
        + balls(0.5 + 2.0 ** -13),
        # exact ties inside the stack: the rect on the coat's lower face, in either order; the coat twice
        "coplanar_rb": lambda: slab(0.0, sep=0.0) + balls(0.0),
        "coplanar_br": lambda: slab(0.0, sep=0.0)[::-1] + balls(0.0),
        "twin_coats": lambda: slab0 + [coat(-H, 0.0)],
        # no ground stack (kind 1): a sphere's box starts below the top plane; a rect of another orientation; five
        # ground primitives (kGroundMaxPrims = 4); a guard bitmap beyond its size limit
        "sunk": _sunk,
        "wall": lambda: slab0 + [rect_yz(0.0, 1.0, -1.0, 1.0, -3.0, lambertian(0.3, 0.3, 0.3))],
        "five": lambda: _two_coats() + [ground_rect(-0.125)],
        "far": lambda: slab0 + [sphere((40.0, 0.25, 40.0), 0.25, GREY), sphere((-40.0, 0.25, -40.0), 0.25, GREY)],
    }
    return table[name]()


TIE_FREE = ["slab0", "slab_up", "slab_down", "floating", "bare", "neg_radius", "two_coats", "small_coat", "rect_top"]
TIED = ["coplanar_rb", "coplanar_br", "twin_coats"]
KIND2 = TIE_FREE + TIED
KIND1 = ["sunk", "wall", "five", "far"]
NAMES = KIND2 + KIND1
KIND = {**{n: 2 for n in KIND2}, **{n: 1 for n in KIND1}}
# (n, n_box, y_top, guard bitmap present) of the DGround record
RECORD = {"slab0": (2, 1, 0.0, True), "slab_up": (2, 1, 3.0, True), "slab_down": (2, 1, -2.5, True),
          "floating": (2, 1, 0.0, False), "bare": (2, 1, 0.0, False), "neg_radius": (2, 1, 0.0, True),
          "two_coats": (4, 2, 0.0, True), "small_coat": (2, 1, 0.0, True), "rect_top": (3, 1, 0.5001, True),
          "coplanar_rb": (2, 1, 0.0, True), "coplanar_br": (2, 1, 0.0, True), "twin_coats": (3, 2, 0.0, True)}
GUARD_CELLS = (124, 36)  # nx, nz of every scene with guarded balls: 3.75 x 1 between the contact points, 2 cells of margin
# the height the cameras look at: the plane the balls rest on — but rect_top's coat (see cameras)
CAMERA_Y = {"slab_up": 3.0, "slab_down": -2.5}
# (scene, camera) -> the xz the camera centres on where it is not ball 0's contact point.  rect_top's balls rest
# 0.5 above its coat, half way to the `down` camera: centred on any of them the ball and the raised rect hide the
# coat (at most 4 of 16 tiles with 48 coat pixels, tests/test_ground_hop.py test_frames_hold_hop_candidates), and
# no top-plane exit of that scene is a RectBox face, so its guard never decides a hop.  From (-0.375, 0) the raised
# rect's edge at x = -0.5 crosses the left quarter of the frame and no ball is in view.
CAMERA_XZ = {("rect_top", "down"): (-0.375, 0.0)}


def scene_json(name):
    return json.dumps({"skybox": "Above", "objects": objects(name)})


def scene(name):
    return rt.SceneBuilder.from_json(scene_json(name)).finalize(SEED)


def cameras(name):
    """{"down": straight down from 1.25 above the contact point of ball 0, "low": from 7 degrees of elevation at
    0.875 from it} — tests/test_gpu_hop_ground.py guard_cameras on this family: the ball's cap or flank in the
    middle of a frame of coat, so guarded exits and served ones fall in the same waves.  rect_top's cameras look
    at its coat (y = 0), not at the plane its balls rest on: the raised rect covers a part of the view."""
    import numpy as np
    y = CAMERA_Y.get(name, 0.0)
    x, z = CAMERA_XZ.get((name, "down"), ball_xz(0))
    down = rt.CameraBuilder(width=32, aspect_ratio=(32, 32), vfov=30.0, focal_length=1.0, aperture=0.001).build(
        rt.CameraPosition((x, y + 1.25, z), (x, y, z), (0.0, 0.0, -1.0), focus_length=1.25))
    x, z = CAMERA_XZ.get((name, "low"), ball_xz(0))
    e = np.radians(7.0)
    low = rt.CameraBuilder(width=32, aspect_ratio=(32, 32), vfov=8.0, focal_length=1.0, aperture=0.001).build(
        rt.CameraPosition((x + 0.875 * np.cos(e), y + 0.875 * np.sin(e), z), (x, y, z), (0.0, 1.0, 0.0), focus_length=0.875))
    assert (down.image_width, down.image_height, low.image_width, low.image_height) == (32, 32, 32, 32)
    return {"down": down, "low": low}


def write_prims(finalized, path):
    """tests/ground_hop_check.c's input: one line per primitive of a finalized scene — kind, dielectric, p0 .. p5
    as hex floats."""
    from raytracer import _native as N
    d = finalized.desc
    kinds = {N.RT_GEOM_SPHERE: 0, N.RT_GEOM_RECT_XZ: 3, N.RT_GEOM_RECT_BOX: 4}
    with open(path, "w") as f:
        for i in range(d.n_objects):
            o = d.objects[i]
            diel = int(d.materials[o.material].kind == N.RT_MAT_DIELECTRIC)
            f.write(" ".join([str(kinds[o.geometry]), str(diel)] + [float(o.p[k]).hex() for k in range(6)]) + "\n")
