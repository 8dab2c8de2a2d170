"""The rules of an adaptive frame on the CPU (csrc/rt/adaptive.h through tools/adaptive_check): argument
validation, the step schedule, list compaction and the tile error with its stop rule.  The tool is built
twice: plainly, and as a stand-alone program with AddressSanitizer + UBSan (every case runs on both)."""
import math
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "adaptive_check.cpp")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adaptive") / ("adaptive_check_" + request.param))
    flags = ["-O1"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, SRC], check=True, timeout=180)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True, timeout=60)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return [ln for ln in out.stdout.split("\n") if ln.strip()]
    return run


def schedule(tool, samples, chunk, mn, step):
    return [tuple(map(int, ln.split())) for ln in tool("schedule", samples, chunk, mn, step)]


def test_schedule_clips_at_the_maximum(tool):
    assert schedule(tool, 32, 4, 8, 8) == [(0, 8), (8, 16), (16, 24), (24, 32)]
    assert schedule(tool, 28, 4, 8, 8) == [(0, 8), (8, 16), (16, 24), (24, 28)]   # the last step is clipped
    assert schedule(tool, 8, 4, 8, 8) == [(0, 8)]                                  # min == max: one step
    assert schedule(tool, 12, 0, 8, 64) == [(0, 8), (8, 12)]                       # batch 0 -> 4; step > rest
    s = schedule(tool, 10000, 16, 64, 48)
    assert s[0] == (0, 64) and s[-1][1] == 10000 and all(a[1] == b[0] for a, b in zip(s, s[1:]))
    assert all(e - b == 48 for b, e in s[1:-1]) and 0 < s[-1][1] - s[-1][0] <= 48
    # every range is a whole number of batches (the fold counts one batch per chunk)
    assert all(b % 16 == 0 and e % 16 == 0 for b, e in s)


GOOD = dict(samples=32, chunk=4, begin=0, count=0, world=1, mn=8, step=8, thr=0.05, floor=0.01)


def validate(tool, **kw):
    a = {**GOOD, **kw}
    return tool("validate", a["samples"], a["chunk"], a["begin"], a["count"], a["world"], a["mn"], a["step"],
                a["thr"], a["floor"])[0]


def test_validation_accepts_the_documented_calls(tool):
    assert validate(tool) == "ok 4"
    assert validate(tool, chunk=0) == "ok 4"          # sample_chunk 0 means 4
    assert validate(tool, chunk=8, mn=16) == "ok 8"
    assert validate(tool, thr=0.0) == "ok 4"          # never stop
    assert validate(tool, thr="inf") == "ok 4"        # stop at min_samples
    assert validate(tool, floor=0.0) == "ok 4"
    assert validate(tool, mn=32) == "ok 4"            # min_samples == samples


@pytest.mark.parametrize("bad", [
    dict(step=6), dict(step=0), dict(step=-8),                 # step: a positive multiple of the batch
    dict(mn=4), dict(mn=10), dict(mn=0), dict(mn=40),          # min_samples: >= 2 batches, a multiple, <= samples
    dict(samples=30), dict(samples=0),                         # samples: a positive multiple of the batch
    dict(begin=4), dict(count=8),                              # no sample range
    dict(world=2), dict(world=0),                              # no tile sharding
    dict(chunk=-1), dict(chunk=3),                             # (32 is no multiple of 3)
    dict(thr=-0.1), dict(thr="nan"), dict(floor=-1.0), dict(floor="inf"), dict(floor="nan"),
])
def test_validation_refuses_each_bad_argument(tool, bad):
    assert validate(tool, **bad).startswith("invalid ")


def test_compaction_keeps_ascending_order(tool):
    thr = 0.5
    tiles = [(0, 0.1), (3, 0.7), (4, 0.5), (9, float("nan")), (10, 0.50000001), (17, 0.0), (23, float("inf")), (24, 2.0)]
    out = tool("compact", thr, *[f"{t}:{e!r}" for t, e in tiles])
    kept = list(map(int, out[0].split())) if out else []
    assert kept == [3, 9, 10, 23, 24]          # !(e <= threshold): NaN goes on, e == threshold stops
    assert kept == sorted(kept)
    # threshold 0 keeps every tile (also one without variance: that frame is the uniform frame), +inf only NaN
    assert list(map(int, tool("compact", 0, "1:0.25", "2:0", "5:1e-300")[0].split())) == [1, 2, 5]
    assert list(map(int, tool("compact", "inf", "1:0.25", "2:nan", "5:inf")[0].split())) == [2]
    assert tool("compact", 0.5, "1:0.25") == []


def tile_error(tool, n, b, floor, pix):
    out = tool("error", n, b, floor, *[f"{float(m1)!r}:{float(m2)!r}" for m1, m2 in pix])
    v = [float(x) for x in out[:len(pix)]]
    E, M, e = map(float, out[len(pix)].split())
    return v, E, M, e, out[len(pix) + 1]


def test_error_formula(tool):
    rng = np.random.default_rng(5)
    n, b, floor = 6, 4, 0.01
    y = rng.uniform(0.0, 3.0, size=(40, n)) * b        # batch sums' r+g+b of 40 in-image pixels of an edge tile
    m1, m2 = y.sum(axis=1), (y * y).sum(axis=1)
    v, E, M, e, verdict = tile_error(tool, n, b, floor, list(zip(m1, m2)))
    v_ref = np.maximum(0.0, m2 - m1 * m1 / n) / (n - 1)
    assert np.allclose(v, v_ref, rtol=1e-13, atol=0)
    assert np.allclose(v, y.var(axis=1, ddof=1), rtol=1e-9)          # it is the batch sums' sample variance
    K, N = len(y), n * b
    e_ref = math.sqrt(n * v_ref.sum() / K) / (m1.sum() / K + N * floor)
    assert math.isclose(E, v_ref.sum(), rel_tol=1e-13) and math.isclose(M, m1.sum(), rel_tol=1e-13)
    assert math.isclose(e, e_ref, rel_tol=1e-12)
    assert verdict == ("continues" if not e_ref <= 0.5 else "stops")
    # m2 - m1^2 / n below 0 (rounding can leave it there for equal observations) is clamped to 0
    v, E, _, e, verdict = tile_error(tool, 3, 4, 0.01, [(0.3, 0.0299)])
    assert v == [0.0] and E == 0.0 and e == 0.0 and verdict == "stops"


def test_error_of_a_black_tile_is_zero(tool):
    # no variance: e = 0 whatever the mean, also with mean 0 and no noise floor (0 / 0 otherwise) — so a
    # max_depth == 0 frame stops at min_samples
    for floor in (0.0, 0.01):
        _, E, M, e, verdict = tile_error(tool, 2, 4, floor, [(0.0, 0.0)] * 64)
        assert (E, M, e, verdict) == (0.0, 0.0, 0.0, "stops")


def test_error_is_nan_for_one_batch_and_for_nan_moments(tool):
    # n = 1: no variance estimate, the tile never converges
    v, _, _, e, verdict = tile_error(tool, 1, 4, 0.01, [(1.0, 1.0), (2.0, 4.0)])
    assert all(math.isnan(x) for x in v) and math.isnan(e) and verdict == "continues"
    # a NaN radiance stays NaN through the clamp and keeps the tile rendering
    v, E, _, e, verdict = tile_error(tool, 4, 4, 0.01, [(1.0, 1.0), (float("nan"), float("nan"))])
    assert not math.isnan(v[0]) and math.isnan(v[1]) and math.isnan(E) and math.isnan(e) and verdict == "continues"
    v, _, _, e, verdict = tile_error(tool, 4, 4, 0.01, [(1.0, float("inf"))])
    assert v == [math.inf] and verdict == "continues"
