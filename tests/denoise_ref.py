"""Shared by tests/test_denoise.py and tests/test_gpu_denoise.py: seeded synthetic frames for the à-trous
filter and a numpy restatement of its definition (include/shirley_rt.h, ABI 10), vectorised per tap and
accumulated in tap order (dy outer, dx inner), so that it reproduces rt_denoise bit for bit."""
import numpy as np

import raytracer as rt

KH = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)

SIZES = [(37, 21), (8, 8)]
ITERATIONS = [0, 1, 3, 6]  # stride 32 in the sixth iteration exceeds the 37x21 frame: every far tap is skipped


def synthetic(width, height, seed=7, samples=16, feature_samples=4):
    """A frame of three surfaces (two tilted planes and a sky band) with noisy colour: dict of accum, albedo,
    normal, depth sums, per-pixel counts (one of them 0), variance and the two sample counts."""
    rng = np.random.default_rng(seed)
    h, w = height, width
    yy, xx = np.mgrid[0:h, 0:w]
    region = np.where(yy >= (3 * h) // 4, 2, np.where(xx + yy // 2 < w // 2, 0, 1))  # 2: sky
    n = np.zeros((h, w, 3))
    n[region == 0] = np.array([0.0, 0.6, 0.8])
    n[region == 1] = np.array([0.8, 0.0, -0.6])
    n += np.where((region != 2)[..., None], rng.normal(0.0, 0.02, (h, w, 3)), 0.0)
    z = np.where(region == 0, 5.0 + 0.05 * xx, np.where(region == 1, 7.5 + 0.03 * yy, 0.0))
    a = np.where((region == 0)[..., None], [0.7, 0.3, 0.2], np.where((region == 1)[..., None], [0.2, 0.6, 0.7],
                                                                      [0.6, 0.7, 1.0]))
    a = a * (1.0 + 0.02 * rng.standard_normal((h, w, 1)))
    a[0, 0] = 0.0  # below the albedo floor
    light = 0.3 + 0.7 * (xx / max(1, w - 1))
    mean = a * light[..., None] * (1.0 + 0.35 * rng.standard_normal((h, w, 3)))
    counts = rng.choice([8, 16, 24], size=(h, w)).astype(np.int32)
    counts[h // 2, w // 3] = 0
    var = (0.35 * light * a.sum(axis=-1)) ** 2 / np.maximum(counts, 1) * rng.uniform(0.5, 1.5, (h, w))
    fs = feature_samples
    return dict(width=w, height=h, samples=samples, feature_samples=fs,
                accum_counts=np.ascontiguousarray(mean * counts[..., None]),
                accum_scalar=np.ascontiguousarray(mean * samples),
                albedo=np.ascontiguousarray(a * fs), normal=np.ascontiguousarray(n * fs),
                depth=np.ascontiguousarray(z * fs), counts=counts, variance=np.ascontiguousarray(var))


def case_arrays(frame, use_counts, use_variance):
    """(accum, kwargs of rt.denoise) for one of the four input forms of a synthetic frame"""
    kw = dict(samples=frame["samples"], feature_samples=frame["feature_samples"])
    if use_counts:
        kw["counts"] = frame["counts"]
    if use_variance:
        kw["variance"] = frame["variance"]
    return frame["accum_counts" if use_counts else "accum_scalar"], kw


def dmax(a, b):
    """denoise.h's dn_max: a > b ? a : b"""
    return np.where(a > b, a, b)


def f_edge(x):
    t = dmax(0.0, 1.0 - x)
    return t * t


def finite(x):
    return (x - x) == 0.0


def numpy_denoise(accum, albedo, normal, depth, samples=0, feature_samples=0, settings=None, counts=None,
                  variance=None):
    S = settings or rt.DenoiseSettings()
    accum = np.asarray(accum, dtype=np.float64)
    h, w, _ = accum.shape
    if S.iterations == 0:
        return accum.copy()
    fs = float(feature_samples or samples)
    cnt = np.full((h, w), samples, dtype=np.int32) if counts is None else np.asarray(counts, dtype=np.int32)
    live = cnt > 0
    nf = cnt.astype(np.float64)
    has_var = variance is not None
    with np.errstate(all="ignore"):
        a = albedo / fs
        A = dmax(a, S.albedo_floor)
        c = np.where(live[..., None], (accum / nf[..., None]) / A, 0.0)
        m = ((A[..., 0] * A[..., 0] + A[..., 1] * A[..., 1]) + A[..., 2] * A[..., 2]) / 3.0
        var = np.where(live, variance / m, 0.0) if has_var else np.zeros((h, w))
        z = depth / fs
        n = normal / fs
        nn = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        for it in range(S.iterations):
            s = 1 << it
            usable = live & finite(c[..., 0]) & finite(c[..., 1]) & finite(c[..., 2])
            sc = np.zeros((h, w, 3))
            sw = np.zeros((h, w))
            sv = np.zeros((h, w))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = dy * s, dx * s
                    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    if dx == 0 and dy == 0:
                        wgt = np.ones((y1 - y0, x1 - x0))
                        use = np.ones((y1 - y0, x1 - x0), dtype=bool)
                    else:
                        use = usable[Q]
                        dot = (n[P][..., 0] * n[Q][..., 0] + n[P][..., 1] * n[Q][..., 1]) + n[P][..., 2] * n[Q][..., 2]
                        d = dmax(0.0, dot)
                        wn = (d * d) / (nn[P] * nn[Q])
                        for _ in range(S.normal_power_log2):
                            wn = wn * wn
                        pz, qz = nn[P] == 0.0, nn[Q] == 0.0
                        wn = np.where(pz & qz, 1.0, np.where(pz | qz, 0.0, wn))
                        r = (z[P] - z[Q]) / (S.sigma_z * (z[P] + z[Q]) + 1e-300)
                        wz = f_edge(r * r)
                        da = a[P] - a[Q]
                        wa = f_edge(((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]) /
                                    (S.sigma_a * S.sigma_a))
                        wgt = (wn * wz) * wa
                        if has_var:
                            dc = c[P] - c[Q]
                            wc = f_edge(((dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]) /
                                        ((S.sigma_c * S.sigma_c) * (var[P] + var[Q]) + 1e-300))
                            wgt = wgt * wc
                    hw = (KH[dy + 2] * KH[dx + 2]) * wgt
                    sc[P] += np.where(use[..., None], hw[..., None] * c[Q], 0.0)
                    sw[P] += np.where(use, hw, 0.0)
                    sv[P] += np.where(use, (hw * hw) * var[Q], 0.0)
            c = np.where(usable[..., None], sc / sw[..., None], c)
            var = np.where(usable, sv / (sw * sw), var)
        return np.where(live[..., None], (c * A) * nf[..., None], 0.0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
