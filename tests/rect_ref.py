"""Solid-angle sampling of rect lights (rt_scene_light_sampling, mode RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL;
include/shirley_rt.h) restated from the header's text in Python floats (IEEE binary64, math.sqrt
correctly rounded, nothing fused): the portable sin, cos, atan2 and acos the definition names (csrc/rt/portable_libm.h,
portable_trig.h) operation for operation, the spherical rectangle and its sample, and tests/cone_ref.py's record,
light sample, rt_render_nee and rt_render_direct restatements with the third mode.  cone_ref's functions are wrapped,
not edited: in modes AREA and CONE, and for a sphere light in mode ALL, everything here is cone_ref's."""
import contextlib
import math

import numpy as np

import cone_ref as K
import oracle_lib as O
from direct_ref import PI, RECTS, _dot
from raytracer import _native as N

AREA, CONE, ALL = K.AREA, K.CONE, N.RT_LIGHT_SAMPLE_SOLID_ANGLE_ALL
CUT, INSIDE, COPLANAR, SMALL = 1, 2, 4, 8  # rt_light_sample.flags
ZERO = CUT | INSIDE | COPLANAR
NAN, INF = float("nan"), float("inf")
TWOPI = 6.283185307179586
MIN_S = 2.0 ** -20
HV_GUARD = 1.0 - 2.0 ** -40


def fdiv(a, b):
    """IEEE a / b (Python raises where the quotient is an infinity or a NaN)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


# ---- portable_libm.h / portable_trig.h ---------------------------------------------------------------
_S = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04,
      2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10)
_C = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05,
      -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11)


def _sin_cos(x):
    """(k, sin kernel, cos kernel) of pl_sin's reduction: k = rint(x 2/pi), ties to even."""
    k = float(round(x * 6.36619772367581382433e-01))
    r = ((x - k * 1.57079632673412561417e+00) - k * 6.07710050630396597660e-11) - k * 2.02226624871116645580e-21
    z = r * r
    s = r + (r * z) * (_S[0] + z * (_S[1] + z * (_S[2] + z * (_S[3] + z * (_S[4] + z * _S[5])))))
    c = (1.0 - 0.5 * z) + (z * z) * (_C[0] + z * (_C[1] + z * (_C[2] + z * (_C[3] + z * (_C[4] + z * _C[5])))))
    return int(k) & 3, s, c


def pl_sin(x):
    if not abs(x) <= 1e9:
        return NAN if (x != x or abs(x) == INF) else 0.0
    q, s, c = _sin_cos(x)
    return (s, c, -s, -c)[q]


def pl_cos(x):
    if not abs(x) <= 1e9:
        return NAN if (x != x or abs(x) == INF) else 0.0
    q, s, c = _sin_cos(x)
    return (c, -s, -c, s)[q]


def pl_atan01(t):
    base = 0.0
    if t > 0.26794919243112270:
        sq3 = 1.73205080756887719318
        t = (sq3 * t - 1.0) / (sq3 + t)
        base = 5.23598775598298815658e-01
    z = t * t
    p = 1.0 / 25.0
    for odd in (23.0, 21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = 1.0 / odd - z * p
    return base + (t - (t * z) * p)


def _neg(v):
    return math.copysign(1.0, v) < 0.0


def pl_atan2(y, x):
    pi, pio2 = 3.14159265358979311600e+00, 1.57079632679489655800e+00
    if x != x or y != y:
        return NAN
    ax, ay = abs(x), abs(y)
    if ax == 0.0 and ay == 0.0:
        return (pi if _neg(x) else 0.0) * (-1.0 if _neg(y) else 1.0)
    a = pl_atan01(ay / ax) if ay <= ax else pio2 - pl_atan01(ax / ay)
    if _neg(x):
        a = pi - a
    return -a if _neg(y) else a


def pl_acos(x):
    if not abs(x) <= 1.0:
        return NAN
    return pl_atan2(math.sqrt((1.0 - x) * (1.0 + x)), x)


# ---- the spherical rectangle ------------------------------------------------------------------------
class View:
    """x0, x1, y0, y1, z0 (negated where positive: flip), and for z0 != 0: b0, b1, k, S."""


def rect_view(geom, p, x):
    d1, d2, axis = RECTS[geom]
    v = View()
    v.x0, v.x1 = p[0] - x[d1], p[1] - x[d1]
    v.y0, v.y1 = p[2] - x[d2], p[3] - x[d2]
    z0 = p[4] - x[axis]
    v.flip, v.z0, v.S = False, z0, None
    if z0 == 0.0:
        return v
    if z0 > 0.0:
        z0 = -z0
        v.flip = True
    v.z0 = z0
    zz = z0 * z0
    b0 = fdiv(-v.y0, math.sqrt(zz + v.y0 * v.y0))
    n1z = fdiv(v.x1, math.sqrt(zz + v.x1 * v.x1))
    b1 = fdiv(v.y1, math.sqrt(zz + v.y1 * v.y1))
    n3z = fdiv(-v.x0, math.sqrt(zz + v.x0 * v.x0))
    g0 = pl_acos(-(b0 * n1z))
    g1 = pl_acos(-(n1z * b1))
    g2 = pl_acos(-(b1 * n3z))
    g3 = pl_acos(-(n3z * b0))
    v.b0, v.b1 = b0, b1
    v.k = (TWOPI - g2) - g3
    v.S = (g0 + g1) - v.k
    return v


def rect_point(v, u, t):
    """(w[d1], w[d2], w[axis]) of an open view for the draws (u, t)."""
    au = u * v.S + v.k
    fu = fdiv(pl_cos(au) * v.b0 - v.b1, pl_sin(au))
    cu = fdiv(1.0, math.sqrt(fu * fu + v.b0 * v.b0))
    cu = cu if fu > 0.0 else -cu
    cu = -1.0 if cu < -1.0 else 1.0 if cu > 1.0 else cu
    xu = fdiv(-(cu * v.z0), math.sqrt(1.0 - cu * cu))
    xu = v.x0 if xu < v.x0 else v.x1 if xu > v.x1 else xu
    dd = xu * xu + v.z0 * v.z0
    d = math.sqrt(dd)
    h0 = fdiv(v.y0, math.sqrt(dd + v.y0 * v.y0))
    h1 = fdiv(v.y1, math.sqrt(dd + v.y1 * v.y1))
    hv = h0 + t * (h1 - h0)
    hv2 = hv * hv
    yv = fdiv(hv * d, math.sqrt(1.0 - hv2)) if hv2 < HV_GUARD else v.y1
    return xu, yv, (-v.z0 if v.flip else v.z0)


def solid_angle_atan(geom, p, x):
    """The rect's solid angle by the closed atan form (a check of S, not part of the definition)."""
    v = rect_view(geom, p, x)
    z = abs(v.z0)

    def corner(a, b):
        return math.atan2(a * b, z * math.sqrt((a * a + b * b) + z * z))
    return (corner(v.x1, v.y1) - corner(v.x0, v.y1)) - (corner(v.x1, v.y0) - corner(v.x0, v.y0))


# ---- the light sample -------------------------------------------------------------------------------
def _count(ref, name):
    if ref is not None:
        setattr(ref, name, getattr(ref, name, 0) + 1)


def sample_point(grid, lights, mode, seed, pixel, s, draw, x, n, ref=None):
    """cone_ref.sample_point with the third mode: a rect light's sample in mode ALL is restated here, everything
    else is cone_ref's (a sphere light in mode ALL is its mode CONE).  The sample carries S in `om` and `rect`."""
    rng = O.lib().or_rng_f64
    nl = float(len(lights))
    if grid is not None:
        cell = grid.cell(x)
        k, pk = grid.pick(cell, rng(seed, pixel, s, draw))
    else:
        cell, pk = 0, 1.0
        k = min(int(rng(seed, pixel, s, draw) * nl), len(lights) - 1)
    _, geom, emitter, p, area, colour = lights[k]
    if mode != ALL or geom == N.RT_GEOM_SPHERE:
        out = K.sample_point(grid, lights, CONE if mode == ALL else mode, seed, pixel, s, draw, x, n, ref)
        out.rect = False
        return out
    draw += 1
    out = K.Sample()
    out.cell, out.pk, out.k, out.om, out.d2, out.cone, out.rect = cell, pk, k, 0.0, 0.0, False, False
    if ref is not None:
        ref.kinds[(geom, emitter)] = ref.kinds.get((geom, emitter), 0) + 1
    d1, d2, axis = RECTS[geom]
    v = rect_view(geom, p, x)
    if v.S is None:
        _count(ref, "coplanar")
        out.flags, out.draw, out.w, out.cx, out.cy = COPLANAR, draw, [0.0, 0.0, 0.0], 0.0, 0.0
        return out
    u = rng(seed, pixel, s, draw)
    t = rng(seed, pixel, s, draw + 1)
    draw += 2
    w = [0.0, 0.0, 0.0]
    if v.S >= MIN_S:
        _count(ref, "rect_angle")
        out.rect, out.om, small = True, v.S, 0
        w[d1], w[d2], w[axis] = rect_point(v, u, t)
    else:
        _count(ref, "fallback")
        small = SMALL
        w[d1] = (p[0] + u * (p[1] - p[0])) - x[d1]
        w[d2] = (p[2] + t * (p[3] - p[2])) - x[d2]
        w[axis] = p[4] - x[axis]
    dd = _dot(w, w)
    dist = math.sqrt(dd)
    if dist == 0.0 or dist != dist:
        cx = cy = NAN
    else:
        cx = _dot(n, w) / dist
        cy = abs(w[axis]) / dist
    out.draw, out.w, out.cx, out.cy, out.d2 = draw, w, cx, cy, dd
    out.flags = (0 if (cx > 0.0 and cy > 0.0) else CUT) | small
    return out


def g_factor(sm, lights, mis, grid_pick):
    if not sm.rect:
        return K.g_factor(sm, lights, mis, grid_pick)
    nl = float(len(lights))
    if mis:
        gs = sm.cx / PI
        pl = sm.pk / sm.om if grid_pick else 1.0 / (sm.om * nl)
        return gs / (pl + gs)
    return sm.cx * ((sm.om / sm.pk if grid_pick else sm.om * nl) / PI)


def record(grid, lights, mode, seed, i, x, n):
    """cone_ref.record with the third mode."""
    sm = sample_point(grid, lights, mode, seed, i, 0, 0, x, n)
    g = [0.0, 0.0] if sm.flags & ZERO else [g_factor(sm, lights, mis, grid is not None) for mis in (False, True)]
    return (sm.k, sm.flags, sm.draw, sm.w[0], sm.w[1], sm.w[2], sm.cx, sm.cy, g[0], g[1])


def light_sample(grid, lights, mode, seed, pixel, s, draw, x, n, a, shadow, mis, ref=None):
    """cone_ref.light_sample with the third mode."""
    sm = sample_point(grid, lights, mode, seed, pixel, s, draw, x, n, ref)
    zero = [0.0, 0.0, 0.0]
    if sm.flags & ZERO:
        if ref is not None and sm.flags & CUT:
            ref.cut += 1
        return zero, sm.draw, sm.cell
    occ = shadow(list(x) + sm.w)
    if ref is not None:
        ref.occluded += occ
        ref.unoccluded += not occ
    if occ:
        return zero, sm.draw, sm.cell
    _, _, emitter, _, _, colour = lights[sm.k]
    le = [c * sm.cy for c in colour] if emitter == N.RT_MAT_FAIRY_LIGHT else colour
    g = g_factor(sm, lights, mis, grid is not None)
    return [(a[c] * le[c]) * g for c in range(3)], sm.draw, sm.cell


_cone_emission_weight = K.emission_weight  # (cone_ref's own, whatever _third_mode() puts in its place)


def emission_weight(grid, lights, mode, mis, lj, cell_prev, cxp, origin, dv, normal, t):
    """cone_ref.emission_weight with the third mode: a listed rect hit in mode ALL."""
    _, geom, _, p, area, _ = lights[lj]
    if mode != ALL:
        return _cone_emission_weight(grid, lights, mode, mis, lj, cell_prev, cxp, origin, dv, normal, t)
    if geom == N.RT_GEOM_SPHERE:
        return _cone_emission_weight(grid, lights, CONE, mis, lj, cell_prev, cxp, origin, dv, normal, t)
    v = rect_view(geom, p, origin)
    if v.S is None or not cxp > 0.0:
        return 1.0
    if not v.S >= MIN_S:
        return _cone_emission_weight(grid, lights, AREA, mis, lj, cell_prev, cxp, origin, dv, normal, t)
    if not mis:
        return 0.0
    gs = cxp / PI
    pl = grid.prob(cell_prev, lj) / v.S if grid is not None else 1.0 / (v.S * float(len(lights)))
    return gs / (pl + gs)


@contextlib.contextmanager
def _third_mode():
    """cone_ref's frame loops call its light_sample and emission_weight by name: hand them the wrappers above."""
    saved = K.light_sample, K.emission_weight
    K.light_sample, K.emission_weight = light_sample, emission_weight
    try:
        yield
    finally:
        K.light_sample, K.emission_weight = saved


def _with_counts(ref):
    for name in ("coplanar", "rect_angle", "fallback"):
        setattr(ref, name, getattr(ref, name, 0))
    return ref


def oracle_nee(scene, cam, seed, s_begin, s_end, max_depth, mis, cells, mode, osc=None, stats=True):
    """cone_ref.oracle_nee with the third mode; the frame also counts rect samples by solid angle (rect_angle),
    rect samples that fell back to the area form (fallback) and coplanar vertices."""
    with _third_mode():
        return _with_counts(K.oracle_nee(scene, cam, seed, s_begin, s_end, max_depth, mis, cells, mode, osc, stats))


def oracle_direct(scene, cam, seed, s_begin, s_end, chain, cells, mode, osc=None):
    with _third_mode():
        return _with_counts(K.oracle_direct(scene, cam, seed, s_begin, s_end, chain, cells, mode, osc))


# ---- the vertex set of the record tests -------------------------------------------------------------
EDGES = ("coplanar", "z+", "z-", "corner", "centre", "near10", "near40", "horizon", "S+", "S-")


def edge_vertices(geom, p):
    """(name, x, n) per entry of EDGES for the rect light (geom, p), with e its longer side and c its centre: a vertex
    in the rect's plane (z0 == 0 exactly); one on either side of it (z0 > 0: flipped; z0 < 0); one straight under the
    corner (d1_min, d2_min), so x0 == 0 and y0 == 0 exactly; one under the centre; under the centre at e 2^-10 and
    e 2^-40 from the plane; under the centre with a normal along d1, whose horizon cuts the rect in two; and on the
    axis through the centre where area / distance^2 = 2^-20 * 1.01 and 2^-20 * 0.99 (S just above and just below
    the bound: at that distance S is area / distance^2 to 1e-6 relative)."""
    d1, d2, axis = RECTS[geom]
    e = max(p[1] - p[0], p[3] - p[2])
    c1, c2 = p[0] + (p[1] - p[0]) * 0.5, p[2] + (p[3] - p[2]) * 0.5
    area = (p[1] - p[0]) * (p[3] - p[2])

    def at(a, b, h):
        x = [0.0, 0.0, 0.0]
        x[d1], x[d2], x[axis] = a, b, h
        return x

    def along(i, sign=1.0):
        n = [0.0, 0.0, 0.0]
        n[i] = sign
        return n
    up, down = along(axis), along(axis, -1.0)
    return [
        ("coplanar", at(c1 + e, c2, p[4]), along(d1, -1.0)),
        ("z+", at(c1 + 0.25 * e, c2 - 0.75 * e, p[4] - 1.0), up),
        ("z-", at(c1 + 0.25 * e, c2 - 0.75 * e, p[4] + 1.0), down),
        ("corner", at(p[0], p[2], p[4] - 1.0), up),
        ("centre", at(c1, c2, p[4] - 1.0), up),
        ("near10", at(c1, c2, p[4] - e * 2.0 ** -10), up),
        ("near40", at(c1, c2, p[4] - e * 2.0 ** -40), up),
        ("horizon", at(c1, c2, p[4] - 1.0), along(d1)),
        ("S+", at(c1, c2, p[4] - math.sqrt(area / (MIN_S * 1.01))), up),
        ("S-", at(c1, c2, p[4] - math.sqrt(area / (MIN_S * 0.99))), up),
    ]


def vertex_set(lights, seed, count=2000):
    """cone_ref.vertex_set for rects: slot i's uniform pick on the key (seed, pixel = i, sample 0, draw 0) is known,
    so three slots in four whose pick is a rect light hold that light's next edge vertex (tag: its EDGES name), and
    the others a random vertex of the box [-6, 6] x [-1, 5] x [-6, 6] with a random unit normal (tag None)."""
    rng = O.lib().or_rng_f64
    rs = np.random.RandomState(seed & 0xFFFFFFFF)
    nl = float(len(lights))
    edges = {j: edge_vertices(l[1], l[3]) for j, l in enumerate(lights) if l[1] != N.RT_GEOM_SPHERE}
    used = {j: 0 for j in edges}
    pts, nrm, tags = [], [], []
    for i in range(count):
        k = min(int(rng(seed, i, 0, 0) * nl), len(lights) - 1)
        if k in edges and i % 4 != 3:
            tag, x, n = edges[k][used[k] % len(edges[k])]
            used[k] += 1
        else:
            x = [float(v) for v in rs.uniform([-6.0, -1.0, -6.0], [6.0, 5.0, 6.0])]
            v = rs.normal(size=3)
            n = [float(t) for t in v / np.linalg.norm(v)]
            tag = None
        pts.append(x)
        nrm.append(n)
        tags.append(tag)
    return np.array(pts), np.array(nrm), tags


# ---- expectation ---------------------------------------------------------------------------------
def expectation_figures(make, max_depth, K_, n, seed, cells, modes=(AREA, ALL), flags=(False, True), processes=1):
    """cone_ref.expectation_figures with the third mode."""
    with _third_mode():  # (worker processes are forked inside, so they inherit the wrappers)
        return K.expectation_figures(make, max_depth, K_, n, seed, cells, modes, flags, processes)
