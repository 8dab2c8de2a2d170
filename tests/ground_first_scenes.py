"""Scenes and cameras for the traversal's closed-form answer about a plane stack (rt_device.h plane_first; DESIGN.md
§3.1).  A plain helper (tests/test_ground_first.py on the CPU, tests/test_gpu_ground_first.py on the device), built
on tests/hop_scenes.py's family: all coordinates binary fractions, every stack 8 x 8 around the origin.

  big_ball   slab0 with a glass sphere of radius 1.5 resting on the coat: large enough that the tree keeps it as a
             direct leaf child of the first node a traversal visits, beside the stack's own leaves
             (tests/test_ground_first.py checks that placement on the compiled tree)

cameras(name): 64 x 64 frames —
  down, low  tests/hop_scenes.py's two whole-wave-on-the-coat cameras
  high       straight down from 2^-6 below Y + H (H = 8 on this family: scene_compile.cpp plane_stack), the origin
             height bound; the lens lies in a horizontal plane, so every origin has that height
  above      the same from 2^-6 above it: every camera ray declines by the bound
  grazing    from 2^-9 above the coat along it, 0.05 degrees wide: every slope is beyond the bound (2^10), so whole
             waves decline
  back       pulled back to 14 away, 40 degrees wide: the frame shows the stack's edge, so hit points fall outside
             the core and rays pass over the edge"""
import json

import numpy as np

import hop_scenes as HS
import raytracer as rt

SEED = HS.SEED
HEIGHT = 8.0  # H of every stack here: max(8, twice the sphere boxes' height)
NAMES = ["big_ball"]
CAMERAS = ["down", "low", "high", "above", "grazing", "back"]


def objects(name):
    if name == "big_ball":
        return HS.slab(0.0) + HS.balls(0.0) + [HS.sphere((0.0, 1.5, -2.0), 1.5, HS.glass(1.5))]
    return HS.objects(name)


def scene_json(name):
    return json.dumps({"skybox": "Above", "objects": objects(name)})


def scene(name):
    return rt.SceneBuilder.from_json(scene_json(name)).finalize(SEED)


def _cam(pos, at, vup, vfov, focus):
    cam = rt.CameraBuilder(width=64, aspect_ratio=(64, 64), vfov=vfov, focal_length=1.0, aperture=0.001).build(
        rt.CameraPosition(pos, at, vup, focus_length=focus))
    assert (cam.image_width, cam.image_height) == (64, 64)
    return cam


def cameras(name):
    y = HS.CAMERA_Y.get(name, 0.0)
    x, z = HS.ball_xz(0)
    e = np.radians(7.0)
    north = (0.0, 0.0, -1.0)
    return {
        "down": _cam((x, y + 1.25, z), (x, y, z), north, 30.0, 1.25),
        "low": _cam((x + 0.875 * np.cos(e), y + 0.875 * np.sin(e), z), (x, y, z), (0.0, 1.0, 0.0), 8.0, 0.875),
        "high": _cam((x, y + HEIGHT - 2.0 ** -6, z), (x, y, z), north, 30.0, HEIGHT),
        "above": _cam((x, y + HEIGHT + 2.0 ** -6, z), (x, y, z), north, 30.0, HEIGHT),
        "grazing": _cam((-3.5, y + 2.0 ** -9, 0.0), (3.5, y, 0.0), (0.0, 1.0, 0.0), 0.05, 7.0),
        "back": _cam((10.0, y + 3.0, 10.0), (0.0, y, 0.0), (0.0, 1.0, 0.0), 40.0, 14.0),
    }
