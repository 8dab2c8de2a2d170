"""Scenes for the book-2 primitive forms (rt_device.h ext_t / base_t / ext_record / to_object):
every base shape as a plain surface, an instance, a medium and an instanced medium; enough extended objects to
reach the traversal's inline object test (DExt index >= 32, leaf_tests4); moving spheres under several
shutters; and twin scenes whose frames must be equal bit for bit.  A plain helper with no device import:
tests/test_book2_scenes.py checks these inputs with the oracle alone, tests/test_gpu_book2.py runs them on the
device.

Each builder returns (scene, camera, ray sets).  Every scene has a floor rect and one DiffuseLight rect.  A ray
set is (rays [n][6], t_max); t_min is T_MIN.  Rays are finite with a non-zero direction.  The sets of a scene:

  camera       from around the camera towards points of the scene box
  inside       from inside the scene box, any direction
  objects      towards a point of each object from nearby (every object is the closest hit of some)
  from_inside  from inside each sphere, box and medium, any direction
  axis         towards a point of each object: along an axis (two components exactly 0), or with one
               component exactly 0
  tmax         from around the camera to a point of each object, cut by a finite t_max near that point

Seeds are fixed: a scene, its cameras and its rays are the same in every process."""
import ctypes as C

import numpy as np

import oracle_lib as O
import raytracer as rt
from raytracer import _native as N

SEED = 0x5EED
T_MIN = 0.001
SETS = ("camera", "inside", "objects", "from_inside", "axis", "tmax")
SPHERES = (N.RT_GEOM_SPHERE, N.RT_GEOM_MOVING_SPHERE)
RECT_AXES = {N.RT_GEOM_RECT_XY: (0, 1, 2), N.RT_GEOM_RECT_YZ: (1, 2, 0), N.RT_GEOM_RECT_XZ: (0, 2, 1)}


def solid(r, g, b):
    return rt.TextureLoader.solid(r, g, b)


def lam(r, g, b):
    return rt.Lambertian(solid(r, g, b))


def camera(look_from, look_at, vfov, shutter=(0.0, 0.0), width=32):
    """A pinhole-like camera (aperture 1e-3 as the project's scene cameras have) of a square frame."""
    return rt.CameraBuilder(width=width, aspect_ratio=(1, 1), vfov=vfov, focal_length=1.0, aperture=0.001,
                            shutter=shutter).build(rt.CameraPosition(tuple(look_from), tuple(look_at)))


# ---- geometry of a finalized scene's objects (numpy, for the ray sets and the tests' classification) ----------

def objects(scene):
    d = scene.desc
    return [d.objects[i] for i in range(d.n_objects)]


def uses_uv(desc, ti):
    """oracle.c texture_uses_uv: only an image leaf reads u, v."""
    if ti < 0 or ti >= desc.n_textures:
        return False
    t = desc.textures[ti]
    if t.kind == N.RT_TEX_IMAGE:
        return True
    if t.kind == N.RT_TEX_CHECKER:
        return uses_uv(desc, t.odd) or uses_uv(desc, t.even)
    return False


def is_flattened(scene, i):
    """The rule both sides flatten by (oracle.c flatten_instanced_sphere, scene_compile.cpp flat_object): an instanced
    plain sphere that is no medium, unless it is rotated and its material reads u, v."""
    d = scene.desc
    o = d.objects[i]
    if o.geometry != N.RT_GEOM_SPHERE or not o.transform or o.medium:
        return False
    return o.rotate_y_deg == 0.0 or not uses_uv(d, d.materials[o.material].texture)


def is_extended(scene, i):
    o = scene.desc.objects[i]
    return bool(o.geometry == N.RT_GEOM_MOVING_SPHERE or o.medium or o.transform) and not is_flattened(scene, i)


def ext_index(scene):
    """{object: DExt index}.  scene_compile.cpp numbers the primitives in the reference tree's leaf order, lhs
    before rhs (reference_ranks), and gives the extended ones among them their DExt records in that order — so the
    index is an extended object's rank among the extended objects in leaf order, not in object order."""
    n = C.c_int32(0)
    lib = N.rt_lib()
    assert lib.rt_bvh_build_host(scene.desc_ptr, N.RT_BVH_REFERENCE, C.byref(n), None, None) == 0
    nodes = (N.rt_bvh_node * max(1, n.value))()
    root = C.c_int32(0)
    assert lib.rt_bvh_build_host(scene.desc_ptr, N.RT_BVH_REFERENCE, C.byref(n), nodes, C.byref(root)) == 0
    order, stack = [], [root.value]
    while stack:
        nd = nodes[stack.pop()]
        if nd.leaf >= 0:
            order.append(nd.leaf)
        else:
            stack += [nd.rhs, nd.lhs]
    assert sorted(order) == list(range(scene.desc.n_objects))
    out = {}
    for i in order:
        if is_extended(scene, i):
            out[i] = len(out)
    return out


def bbox(o):
    out = O._d6()
    assert O.lib().or_object_bbox(C.byref(o), out)
    return np.array(list(out))


def to_world(o, p):
    """RotateY::hit and Translate::hit's map of object-frame points [n][3] back to the world."""
    if not o.transform:
        return p
    a = np.radians(o.rotate_y_deg)
    cs, sn = np.cos(a), np.sin(a)
    return np.column_stack([cs * p[:, 0] + sn * p[:, 2], p[:, 1], -sn * p[:, 0] + cs * p[:, 2]]) + np.array(list(o.offset))


def to_object(o, p):
    """The inverse of to_world (tests classify a point as inside an object with it)."""
    if not o.transform:
        return p
    a = np.radians(o.rotate_y_deg)
    cs, sn = np.cos(a), np.sin(a)
    m = p - np.array(list(o.offset))
    return np.column_stack([cs * m[:, 0] - sn * m[:, 2], m[:, 1], sn * m[:, 0] + cs * m[:, 2]])


def center_at_0(o):
    """A sphere's centre as the hit queries see it: they trace at time 0."""
    c0 = np.array(list(o.p[:3]))
    if o.geometry == N.RT_GEOM_SPHERE:
        return c0
    c1, t0, t1 = np.array(list(o.q[:3])), o.q[3], o.q[4]
    return c0 + (c1 - c0) * ((0.0 - t0) / (t1 - t0))


def contains(o, p):
    """Which world points [n][3] lie inside a sphere or a box at time 0 (a rect holds none)."""
    q = to_object(o, p)
    if o.geometry in SPHERES:
        return np.sum((q - center_at_0(o)) ** 2, axis=1) < o.p[3] ** 2
    if o.geometry == N.RT_GEOM_RECT_BOX:
        lo, hi = np.array(list(o.p[:3])), np.array(list(o.p[3:6]))
        return np.all((q > lo) & (q < hi), axis=1)
    return np.zeros(len(p), dtype=bool)


def points_of(o, n, rng):
    """n world points of an object at time 0: in the inner 60 % of a sphere's radius, in a box shrunk by a tenth,
    on a rect a tenth away from its edges."""
    if o.geometry in SPHERES:
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        p = center_at_0(o) + v * (abs(o.p[3]) * 0.6 * rng.uniform(0.2, 1.0, size=(n, 1)))
    elif o.geometry == N.RT_GEOM_RECT_BOX:
        lo, hi = np.array(list(o.p[:3])), np.array(list(o.p[3:6]))
        p = lo + (hi - lo) * rng.uniform(0.1, 0.9, size=(n, 3))
    else:
        a1, a2, ak = RECT_AXES[o.geometry]
        p = np.zeros((n, 3))
        p[:, a1] = o.p[0] + (o.p[1] - o.p[0]) * rng.uniform(0.1, 0.9, size=n)
        p[:, a2] = o.p[2] + (o.p[3] - o.p[2]) * rng.uniform(0.1, 0.9, size=n)
        p[:, ak] = o.p[4]
    return to_world(o, p)


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def ray_sets(scene, look_from, box, seed, per_object=24, n_free=1024):
    """The ray sets of the module docstring.  `box`: the scene box (lo, hi)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(box[0], dtype=float), np.array(box[1], dtype=float)
    objs = objects(scene)
    inf = float("inf")
    sets = {}
    # camera, inside
    orig = np.array(look_from, dtype=float) + rng.normal(scale=0.3, size=(n_free, 3))
    sets["camera"] = (np.hstack([orig, rng.uniform(lo, hi, size=(n_free, 3)) - orig]), inf)
    sets["inside"] = (np.hstack([rng.uniform(lo, hi, size=(n_free, 3)), rng.normal(size=(n_free, 3))]), inf)
    # objects: from 0.5 .. 4 away towards a point of the object, directions of any length
    rows, rows_in, rows_axis, rows_cut = [], [], [], []
    for o in objs:
        target = points_of(o, per_object, rng)
        orig = target + unit(rng, per_object) * rng.uniform(0.5, 4.0, size=(per_object, 1))
        rows.append(np.hstack([orig, (target - orig) * rng.uniform(0.25, 4.0, size=(per_object, 1))]))
        if o.geometry in SPHERES or o.geometry == N.RT_GEOM_RECT_BOX:
            rows_in.append(np.hstack([points_of(o, per_object, rng), rng.normal(size=(per_object, 3))]))
        # axis: the first half along +-e_a from 1 .. 6 away; the second half with component a exactly 0.  The
        # points are moved off the object a little: a ray inside a rect's own plane from a point of that plane is
        # degenerate (0 / 0 in rect.rs:52), which these sets leave out
        target = points_of(o, per_object, rng) + rng.normal(scale=0.05, size=(per_object, 3))
        a = rng.integers(0, 3, size=per_object)
        sign = rng.choice([-1.0, 1.0], size=per_object)
        half = per_object // 2
        d = np.zeros((per_object, 3))
        d[np.arange(half), a[:half]] = sign[:half] * rng.uniform(0.5, 2.0, size=half)
        d[half:] = rng.normal(size=(per_object - half, 3))
        d[np.arange(half, per_object), a[half:]] = 0.0
        dn = d / np.linalg.norm(d, axis=1)[:, None]
        rows_axis.append(np.hstack([target - dn * rng.uniform(1.0, 6.0, size=(per_object, 1)), d]))
        # tmax: the direction ends at the point, t_max in [0.6, 1.2] cuts the ray near it
        target = points_of(o, per_object, rng)
        orig = np.array(look_from, dtype=float) + rng.normal(scale=0.3, size=(per_object, 3))
        rows_cut.append(np.hstack([orig, target - orig]))
    sets["objects"] = (np.vstack(rows), inf)
    sets["from_inside"] = (np.vstack(rows_in), inf)
    sets["axis"] = (np.vstack(rows_axis), inf)
    sets["tmax"] = (np.vstack(rows_cut), 0.9375)
    for name, (rays, _) in sets.items():
        assert np.isfinite(rays).all() and (np.abs(rays[:, 3:]).max(axis=1) > 0).all(), name
        rays.setflags(write=False)
    return sets


FLOOR = (0.5, 0.5, 0.5)


def start(sky, floor, light, light_rgb=(4.0, 4.0, 4.0)):
    """A builder holding the floor rect (object 0) and the DiffuseLight rect (object 1)."""
    b = rt.SceneBuilder()
    b.set_skybox(sky)
    b.add(rt.xz_rect(*floor), lam(*FLOOR))
    b.add(rt.xz_rect(*light), rt.DiffuseLight(solid(*light_rgb)))
    return b


# ---- zoo ------------------------------------------------------------------------------------------------------

ZOO_FROM, ZOO_AT = (0.0, 16.0, -15.0), (0.0, 1.0, 1.0)
ZOO_BOX = ((-9.0, 0.0, -8.0), (9.0, 6.0, 10.0))


def zoo_builder(earth=True):
    """Every base shape as a plain surface and under Transform(rotate_y != 0, offset != 0), angles 30, -18, 135, -25,
    60, 200, 40, -70, 110, 50.  Lambertian or Metal with solid textures, but the instanced spheres' earth texture,
    which keeps them instances (`earth=False` leaves those three out: the scene without a libm call in its paths);
    the solid instanced sphere is flattened."""
    b = start(rt.SkyBox.Above, (-10, 10, -10, 10, 0), (-3, 3, -3, 3, 9))
    T = rt.Transform
    # plain surfaces
    b.add(rt.Sphere((-6, 1, -5), 1.0), lam(0.75, 0.25, 0.25))
    b.add(rt.MovingSphere((-2, 1, -5), (-2, 2, -5), 0.0, 1.0, 1.0), rt.Metal((0.75, 0.75, 0.5), 0.25))
    b.add(rt.RectBox((1, 0, -6), (3, 2, -4)), lam(0.25, 0.75, 0.25))
    b.add(rt.xy_rect(5, 7, 0, 2, -5), rt.Metal((0.5, 0.75, 0.75), 0.0))
    b.add(rt.yz_rect(0, 2, -2, 0, -6), lam(0.25, 0.25, 0.75))
    b.add(rt.xz_rect(-3, -1, -2, 0, 1), rt.Metal((0.75, 0.5, 0.75), 0.5))
    # instances
    b.add(rt.RectBox((-1, 0, -1), (1, 2, 1)), lam(0.75, 0.75, 0.25), transform=T(30.0, (2, 0, -1)))
    b.add(rt.RectBox((-1, 0, -1), (1, 3, 1)), rt.Metal((0.75, 0.75, 0.75), 0.125), transform=T(-18.0, (6, 0, -1)))
    b.add(rt.xy_rect(-1, 1, 0, 2, 0), lam(0.75, 0.5, 0.25), transform=T(135.0, (-6, 0, 3)))
    b.add(rt.yz_rect(0, 2, -1, 1, 0), rt.Metal((0.5, 0.5, 0.75), 0.0), transform=T(-25.0, (-2, 0, 3)))
    b.add(rt.xz_rect(-1, 1, -1, 1, 1), lam(0.25, 0.75, 0.75), transform=T(60.0, (2, 0, 3)))
    b.add(rt.MovingSphere((0, 1, 0), (1, 1, 0), 0.0, 1.0, 1.0), lam(0.75, 0.25, 0.75), transform=T(200.0, (6, 0, 3)))
    if earth:
        e = rt.Lambertian(rt.TextureLoader.EarthBuiltin)
        b.add(rt.Sphere((0, 1, 0), 1.0), e, transform=T(40.0, (-6, 0, 7)))
        b.add(rt.Sphere((0.5, 1, 0), 1.0), e, transform=T(-70.0, (-2, 0, 7)))
        b.add(rt.Sphere((0, 1, 0.5), 1.0), e, transform=T(110.0, (2, 0, 7)))
    b.add(rt.Sphere((0.5, 1, 0), 1.0), lam(0.5, 0.25, 0.25), transform=T(50.0, (6, 0, 7)))
    return b


def zoo(earth=True):
    scene = zoo_builder(earth).finalize(SEED)
    return scene, camera(ZOO_FROM, ZOO_AT, 50.0, shutter=(0.0, 1.0)), ray_sets(scene, ZOO_FROM, ZOO_BOX, 11)


# ---- smoke ----------------------------------------------------------------------------------------------------

SMOKE_FROM, SMOKE_AT = (8.0, 8.0, -20.0), (8.0, 8.0, 0.0)
SMOKE_BOX = ((0.0, 0.0, 0.0), (16.0, 16.0, 16.0))
SMOKE_BOUNDARY_RECT = 11  # the rect given as a medium boundary: never hit


def smoke_builder():
    """A Cornell-style box of side 16 holding the media: two RectBox media at +15 and -18 degrees (a dark and a
    white Isotropic), a sphere, an instanced sphere and a moving sphere; and a rect as a medium boundary, which a
    ray leaves where it enters and so can never scatter in.  Densities 1/8 .. 1/2 against chords of 2 .. 8: rays
    both scatter and pass through."""
    b = start(rt.SkyBox.Nothing, (0, 16, 0, 16, 0), (5, 11, 5, 11, 15), (7.0, 7.0, 7.0))
    T, M = rt.Transform, rt.ConstantMedium
    b.add(rt.xz_rect(0, 16, 0, 16, 16), lam(0.75, 0.75, 0.75))
    b.add(rt.xy_rect(0, 16, 0, 16, 16), lam(0.75, 0.75, 0.75))
    b.add(rt.yz_rect(0, 16, 0, 16, 16), lam(0.125, 0.5, 0.125))
    b.add(rt.yz_rect(0, 16, 0, 16, 0), lam(0.625, 0.0625, 0.0625))
    iso = lambda v: rt.Isotropic(solid(v, v, v))  # noqa: E731
    b.add(rt.RectBox((0, 0, 0), (4, 8, 4)), iso(0.0625), medium=M(0.25), transform=T(15.0, (9, 0, 8)))
    b.add(rt.RectBox((0, 0, 0), (4, 4, 4)), iso(1.0), medium=M(0.375), transform=T(-18.0, (3, 0, 3)))
    b.add(rt.Sphere((12, 12, 6), 2.0), iso(0.75), medium=M(0.5))
    b.add(rt.Sphere((0, 0, 0), 2.0), iso(0.5), medium=M(0.375), transform=T(30.0, (4, 11, 10)))
    b.add(rt.MovingSphere((12, 4, 3), (12, 6, 3), 0.0, 1.0, 2.0), iso(0.875), medium=M(0.4375))
    b.add(rt.xy_rect(2, 6, 9, 13, 6), iso(0.5), medium=M(1.0))
    return b


def smoke():
    scene = smoke_builder().finalize(SEED)
    assert scene.desc.objects[SMOKE_BOUNDARY_RECT].geometry == N.RT_GEOM_RECT_XY
    return scene, camera(SMOKE_FROM, SMOKE_AT, 40.0, shutter=(0.0, 1.0)), ray_sets(scene, SMOKE_FROM, SMOKE_BOX, 12, 40)


# ---- many_ext -------------------------------------------------------------------------------------------------

MANY_FROM, MANY_AT = (0.0, 5.0, -14.0), (0.0, 4.0, 14.0)
MANY_BOX = ((-7.0, 0.0, -2.0), (7.0, 9.0, 34.0))


def many_ext_builder():
    """54 extended objects: eight layers along the view (z = 0, 4, .. 28) of six small objects each, 4 apart, the
    layers staggered in x so that a camera ray passes the bounding boxes of objects of many layers; six media
    among them.  Kinds by position: instanced boxes, instanced rects of the three orientations, moving spheres."""
    b = start(rt.SkyBox.Above, (-12, 12, -6, 34, 0), (-3, 3, 10, 16, 11))
    T, M = rt.Transform, rt.ConstantMedium
    angles = [30.0, -18.0, 135.0, -25.0, 60.0, 200.0, -70.0, 110.0]
    n = 0
    for k in range(8):
        for ix in range(3):
            for iy in range(2):
                x, y, z = 4 * (ix - 1) + (k % 3 - 1), 2 + 4 * iy, 4 * k
                ang = angles[(n + k) % 8]
                col = (0.25 + 0.25 * (n % 3), 0.25 + 0.25 * ((n // 3) % 3), 0.25 + 0.25 * ((n // 9) % 3))
                mat = rt.Metal(col, 0.25) if n % 4 == 3 else lam(*col)
                kind = n % 6
                if n % 9 == 4:  # six media: instanced boxes and moving spheres by turns
                    iso = rt.Isotropic(solid(*col))
                    if (n // 9) % 2 == 0:
                        b.add(rt.RectBox((-1, -1, -1), (1, 1, 1)), iso, medium=M(0.5), transform=T(ang, (x, y, z)))
                    else:
                        b.add(rt.MovingSphere((x, y, z), (x, y + 1, z), 0.0, 1.0, 1.0), iso, medium=M(0.75))
                elif kind == 0:
                    b.add(rt.RectBox((-1, -1, -1), (1, 1, 1)), mat, transform=T(ang, (x, y, z)))
                elif kind == 1:
                    b.add(rt.xy_rect(-1, 1, -1, 1, 0), mat, transform=T(ang, (x, y, z)))
                elif kind == 2:
                    b.add(rt.MovingSphere((x, y, z), (x + 1, y, z), 0.0, 1.0, 0.75), mat)
                elif kind == 3:
                    b.add(rt.yz_rect(-1, 1, -1, 1, 0), mat, transform=T(ang, (x, y, z)))
                elif kind == 4:
                    b.add(rt.xz_rect(-1, 1, -1, 1, 0), mat, transform=T(ang, (x, y, z)))
                else:
                    b.add(rt.RectBox((-1, -0.5, -0.5), (1, 0.5, 0.5)), mat, transform=T(ang, (x, y, z)))
                n += 1
    # six more past the last layer, so that the group of indices >= 32 is no smaller than the other
    for j in range(6):
        x, y, z = 4 * (j % 3 - 1), 3 + 3 * (j // 3), 32
        b.add(rt.MovingSphere((x, y, z), (x, y, z - 1), 0.0, 1.0, 0.75), lam(0.75, 0.5, 0.25))
    return b


def many_ext():
    scene = many_ext_builder().finalize(SEED)
    return scene, camera(MANY_FROM, MANY_AT, 40.0, shutter=(0.0, 1.0)), ray_sets(scene, MANY_FROM, MANY_BOX, 13)


# ---- shutter --------------------------------------------------------------------------------------------------

SHUTTER_FROM, SHUTTER_AT = (0.0, 4.0, -14.0), (0.0, 3.0, 0.0)
SHUTTER_BOX = ((-8.0, 0.0, -4.0), (8.0, 8.0, 6.0))
SHUTTERS = {"open": (0.0, 1.0), "inner": (0.25, 0.75), "frozen": (0.5, 0.5), "frozen0": (0.0, 0.0),
            "frozen1": (1.0, 1.0)}


def shutter_builder():
    """Fast moving spheres (two to four radii per unit of time) over time0 / time1 = (0, 1), and one over (-1, 3):
    its own interval is not the shutter's, so center(t) at t != time0 scales by 1 / 4."""
    b = start(rt.SkyBox.Above, (-12, 12, -8, 10, 0), (-3, 3, -2, 4, 10))
    b.add(rt.MovingSphere((-6, 1, 0), (-2, 1, 0), 0.0, 1.0, 1.0), lam(0.75, 0.25, 0.25))
    b.add(rt.MovingSphere((0, 1, 2), (0, 5, 2), 0.0, 1.0, 1.0), rt.Metal((0.75, 0.75, 0.5), 0.125))
    b.add(rt.MovingSphere((6, 2, -1), (3, 4, 3), 0.0, 1.0, 1.0), lam(0.25, 0.75, 0.25))
    b.add(rt.MovingSphere((-5, 5, 3), (7, 5, 3), -1.0, 3.0, 1.0), lam(0.25, 0.25, 0.75))
    b.add(rt.MovingSphere((-3, 3, -2), (-3, 3, 2), 0.0, 1.0, 0.5), rt.Metal((0.75, 0.5, 0.75), 0.0))
    return b


def shutter(which="open"):
    scene = shutter_builder().finalize(SEED)
    return scene, camera(SHUTTER_FROM, SHUTTER_AT, 40.0, shutter=SHUTTERS[which]), ray_sets(scene, SHUTTER_FROM, SHUTTER_BOX, 14)


SCENES = {"zoo": zoo, "smoke": smoke, "many_ext": many_ext, "shutter": shutter}


# ---- twins ----------------------------------------------------------------------------------------------------

TWIN_FROM, TWIN_AT = (2.0, 5.0, -12.0), (2.0, 2.0, 1.0)
TWIN_OFFSET = (3, 1, -2)
EARTH = "earth"
# the shapes of twins (b) and (c): small integers throughout (a sphere's centre off the origin, so that an offset
# moves it); "earth": the textured sphere
TWIN_SHAPES = {
    "sphere": lambda: rt.Sphere((1, 2, 1), 1.0),
    "earth": lambda: rt.Sphere((1, 2, 1), 1.0),
    "moving": lambda: rt.MovingSphere((0, 2, 1), (2, 3, 1), 0.0, 1.0, 1.0),
    "xy": lambda: rt.xy_rect(0, 3, 1, 3, 1),
    "yz": lambda: rt.yz_rect(1, 3, 0, 2, 1),
    "xz": lambda: rt.xz_rect(0, 3, 0, 2, 2),
    "box": lambda: rt.RectBox((0, 1, 0), (2, 3, 2)),
}


def moved(name, off):
    """Shape `name` of TWIN_SHAPES moved by the integer offset `off`, as a bare shape."""
    dx, dy, dz = off
    return {
        "sphere": lambda: rt.Sphere((1 + dx, 2 + dy, 1 + dz), 1.0),
        "earth": lambda: rt.Sphere((1 + dx, 2 + dy, 1 + dz), 1.0),
        "moving": lambda: rt.MovingSphere((0 + dx, 2 + dy, 1 + dz), (2 + dx, 3 + dy, 1 + dz), 0.0, 1.0, 1.0),
        "xy": lambda: rt.xy_rect(0 + dx, 3 + dx, 1 + dy, 3 + dy, 1 + dz),
        "yz": lambda: rt.yz_rect(1 + dy, 3 + dy, 0 + dz, 2 + dz, 1 + dx),
        "xz": lambda: rt.xz_rect(0 + dx, 3 + dx, 0 + dz, 2 + dz, 2 + dy),
        "box": lambda: rt.RectBox((0 + dx, 1 + dy, 0 + dz), (2 + dx, 3 + dy, 2 + dz)),
    }[name]()


def twin_scene(geometry, material, transform=None, sky=rt.SkyBox.Above):
    b = start(sky, (-10, 14, -10, 14, 0), (-1, 5, -2, 4, 9))
    b.add(geometry, material, transform=transform)
    return b.finalize(SEED)


def twin_material(name):
    return rt.Lambertian(rt.TextureLoader.EarthBuiltin) if name == EARTH else lam(0.75, 0.5, 0.25)


TWINS = ["a"] + [f"b:{s}" for s in TWIN_SHAPES] + [f"c:{s}" for s in TWIN_SHAPES]


def twin(key):
    """(extended scene, its twin, camera) of pair `key`: "a" a MovingSphere under the frozen shutter (1/2, 1/2)
    against the static Sphere at center(1/2); "b:<shape>" the shape under Transform(0, (0, 0, 0)) against the bare
    shape; "c:<shape>" under Transform(0, TWIN_OFFSET) against the bare shape moved by that offset."""
    if key == "a":
        cam = camera(TWIN_FROM, TWIN_AT, 40.0, shutter=(0.5, 0.5))
        m = twin_material("moving")
        return (twin_scene(rt.MovingSphere((0, 1, 0), (4, 3, 2), 0.0, 1.0, 1.0), m),
                twin_scene(rt.Sphere((2, 2, 1), 1.0), m), cam)
    kind, name = key.split(":")
    cam = camera(TWIN_FROM, TWIN_AT, 40.0, shutter=(0.0, 1.0))
    m = twin_material(name)
    off = (0, 0, 0) if kind == "b" else TWIN_OFFSET
    sky = rt.SkyBox.Above
    if key == "c:moving":
        # the one pair whose arithmetic is not exact: a sphere's normal (p - c) / r carries the rounding of the hit
        # point, which o - offset changes (the camera's origin is no integer), and a moved sphere that stays an
        # instance is the moving one.  So this pair is equal in what its paths meet, not in their last bits: under a
        # flat sky every colour is a product of albedos and of the sky's or the light's emission, whatever the
        # direction.  Frozen at the dyadic 1 / 4.
        cam = camera(TWIN_FROM, TWIN_AT, 40.0, shutter=(0.25, 0.25))
        sky = rt.SkyBox.Flat((0.5, 0.75, 1.0))
    return (twin_scene(TWIN_SHAPES[name](), m, rt.Transform(0.0, off), sky), twin_scene(moved(name, off), m, sky=sky), cam)


# ---- shared, computed once per process and never written to -------------------------------------------------------

OR_HIT = np.dtype(O.or_hit)
_built, _hits = {}, {}


def get(name):
    """SCENES[name]() once per process: (scene, camera, ray sets).  "zoo_solid": the zoo without its earth spheres."""
    if name not in _built:
        _built[name] = zoo(earth=False) if name == "zoo_solid" else SCENES[name]()
    return _built[name]


def oracle_hits(name):
    """{set: or_hit records [n] as a numpy structured array} of scene `name`: ray i of a set traced with
    rt_scene_hit's key for index i, as one device call per set traces it."""
    if name not in _hits:
        scene, _, sets = get(name)
        osc = O.OracleScene(scene)
        out = {}
        for s, (rays, t_max) in sets.items():
            rec = b"".join(bytes(osc.hit(r, T_MIN, t_max, index=i)) for i, r in enumerate(rays))
            out[s] = np.frombuffer(rec, dtype=OR_HIT)
        _hits[name] = out
    return _hits[name]
