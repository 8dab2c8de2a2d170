"""rt_render_nee_adaptive (include/shirley_rt.h) restated in Python over batch frames: B_k is
rt_render_nee's frame over the sample range [k b, (k + 1) b) — from the CPU oracle (nee_ref.oracle_nee) or from the
device's own range calls — and the schedule, the sums, the moments and the tile error are the header's, the error
by the numpy formula of tests/test_gpu_adaptive.py::errors_from_moments.  So that a decision never hangs on a last
bit, m2 is summed with an exactly rounded y * y + m2 (the device's fma) and E, M over the tile's 64 lanes in the
header's six xor rounds; the comparisons of m2 and e keep that test's rtol 1e-9."""
from fractions import Fraction

import numpy as np

import nee_ref as R

RTOL = 1e-9  # m2 and tile_error (tests/test_gpu_adaptive.py's figure); accum, counts and m1 are exact


def oracle_batches(scene, cam, seed, b, n_batches, depth, mis, osc=None):
    out = [R.oracle_nee(scene, cam, seed, k * b, (k + 1) * b, depth, mis, osc, stats=False).sums
           for k in range(n_batches)]
    for a in out:
        a.setflags(write=False)
    return out


def device_batches(gpu, cam, settings_of, b, n_batches, mis):
    """settings_of(**kw) -> RenderSettings with `samples` covering the ranges."""
    out = [gpu.render_nee(cam, settings_of(sample_begin=k * b, sample_count=b), mis=mis) for k in range(n_batches)]
    for a in out:
        a.setflags(write=False)
    return out


class Restated:
    pass


def _fma_sq(y, m2):
    """fma(y, y, m2) element by element: the exact y * y + m2, rounded once (float(Fraction) rounds correctly)."""
    out = []
    for a, c in zip(y.reshape(-1).tolist(), m2.reshape(-1).tolist()):
        exact = np.isfinite(a) and np.isfinite(c)
        out.append(float(Fraction(a) * Fraction(a) + Fraction(c)) if exact else a * a + c)
    return np.array(out).reshape(m2.shape)


def _wave_sum(tile_values):
    """The header's sum over the tile's 64 lanes (lane l = pixel (l % 8, l / 8), absent pixels 0): six rounds
    off = 32 ... 1 in which lane l adds lane l ^ off's value to its own; every lane ends with the same sum."""
    x = np.zeros((8, 8))
    x[:tile_values.shape[0], :tile_values.shape[1]] = tile_values
    x = x.reshape(64)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        x = x + x[lanes ^ off]
    assert (x == x[0]).all() or np.isnan(x).any()
    return float(x[0])


def restate(batches, b, min_samples, step, max_samples, floor, thr):
    """-> accum [H][W][3], counts [H][W], moments [H][W][2], tile_error [TY][TX], checks [(tile, samples, e)]."""
    h, w, _ = batches[0].shape
    tx, ty = (w + 7) // 8, (h + 7) // 8
    r = Restated()
    r.accum = np.zeros((h, w, 3))
    r.counts = np.zeros((h, w), dtype=np.int32)
    r.moments = np.zeros((h, w, 2))
    r.tile_error = np.zeros((ty, tx))
    r.checks = []
    for t in range(tx * ty):
        sl = (slice((t // tx) * 8, min((t // tx) * 8 + 8, h)), slice((t % tx) * 8, min((t % tx) * 8 + 8, w)))
        acc = np.zeros(batches[0][sl].shape)
        m1 = np.zeros(acc.shape[:2])
        m2 = np.zeros(acc.shape[:2])
        n, s_to = 0, min_samples
        while True:
            while n * b < s_to:
                bk = batches[n][sl]
                acc = acc + bk
                y = (bk[..., 0] + bk[..., 1]) + bk[..., 2]
                m1 = m1 + y
                m2 = _fma_sq(y, m2)
                n += 1
            v = np.maximum(0.0, m2 - m1 * m1 / n) / (n - 1)
            E, M, K = _wave_sum(v), _wave_sum(m1), v.size
            e = 0.0 if E == 0.0 else float(np.sqrt(float(n) * E / K) / (M / K + (float(n) * b) * floor))
            r.checks.append((t, n * b, e))
            if not ((not (e <= thr) or thr == 0.0) and n * b < max_samples):
                break
            s_to = min(s_to + step, max_samples)
        r.accum[sl], r.counts[sl], r.tile_error[t // tx, t % tx] = acc, n * b, e
        r.moments[sl] = np.stack([m1, m2], axis=-1)
    return r


def near_tiles(r, thr):
    """Tiles with a checked error within RTOL of the threshold: left out of the decision asserts."""
    return sorted({t for t, _, e in r.checks if np.isfinite(thr) and thr > 0.0 and abs(e - thr) <= RTOL * thr})


def closest(r, thr):
    """The smallest relative distance of a checked, non-zero error from the threshold."""
    d = [abs(e - thr) / thr for _, _, e in r.checks if e > 0.0]
    return min(d) if d else float("inf")


def compare(got, r, thr, label=""):
    """got: Device.render_nee_adaptive's tuple.  accum, counts, m1 exact; m2, tile_error rtol RTOL — for every tile
    not within RTOL of the threshold (at most 1 % of the tiles may be; the caller asserts its inputs leave none)."""
    accum, counts, moments, tile_error, rep = got
    near = near_tiles(r, thr)
    assert len(near) <= 0.01 * r.tile_error.size, f"{label}: {len(near)} tiles on the threshold"
    h, w = counts.shape
    tx = (w + 7) // 8
    keep = np.ones((h, w), dtype=bool)
    for t in near:
        keep[(t // tx) * 8:(t // tx) * 8 + 8, (t % tx) * 8:(t % tx) * 8 + 8] = False
    tkeep = np.ones(r.tile_error.size, dtype=bool)
    tkeep[near] = False
    tkeep = tkeep.reshape(r.tile_error.shape)
    print(f"{label}: tile counts {r.counts[::8, ::8].reshape(-1).tolist()}, closest checked error "
          f"{100.0 * closest(r, thr) if np.isfinite(thr) and thr > 0 else float('nan'):.2f} % from the threshold, "
          f"{len(near)} tiles left out; max rel m2 diff "
          f"{np.max(np.abs(moments[..., 1] - r.moments[..., 1]) / np.maximum(r.moments[..., 1], 1e-300)):.3g}")
    assert np.array_equal(counts[keep], r.counts[keep]), f"{label}: counts"
    assert np.array_equal(accum[keep], r.accum[keep]), f"{label}: accum"
    assert np.array_equal(moments[..., 0][keep], r.moments[..., 0][keep]), f"{label}: m1"
    assert np.allclose(moments[..., 1][keep], r.moments[..., 1][keep], rtol=RTOL, atol=0.0), f"{label}: m2"
    assert np.allclose(tile_error[tkeep], r.tile_error[tkeep], rtol=RTOL, atol=0.0), f"{label}: tile_error"
    return near
