"""ray-cli's adaptive flags on the CPU: what they cannot be combined with is a usage error (exit status 2,
before any device is opened), and the help text names them."""
import os
import subprocess

import pytest

from raytracer import _native as N

CLI = os.path.join(N.BIN_DIR, "ray-cli")
ADAPTIVE = ["render", "random", "-w", "64", "-s", "32", "--adaptive", "0.05"]


@pytest.mark.parametrize("extra,word", [(["--progressive", "2"], "--progressive"), (["--resume", "nowhere.f64"], "--resume"),
                                        (["--gpus", "2"], "one GPU"), (["--dump-accum", "sums.f64"], "checkpoint")])
def test_adaptive_refuses_what_it_does_not_support(extra, word):
    r = subprocess.run([CLI] + ADAPTIVE + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "error: --adaptive" in r.stderr and word in r.stderr


def test_usage_names_the_adaptive_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    for flag in ("--adaptive T", "--min-samples N", "--adaptive-step N", "--noise-floor F"):
        assert flag in r.stderr


def test_missing_value_is_a_usage_error():
    r = subprocess.run([CLI, "render", "random", "--adaptive"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "missing value for --adaptive" in r.stderr
