"""The serve body written out for a y face on the CPU (rt_device.h serve_y).

tests/serve_y_check.c restates the reduced form — front face from the sign of d.y, cos_theta = fmin(|ud.y|, 1), the
reflection and the refraction with the normal's x and z terms dropped, and the hand-back of every lane with a zero or
tiny component — and the general serve body from the oracle's own record, refract, reflect and Schlick functions, and
compares every output bit on 2 M adversarial cases per index."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_INDEX = 2_000_000
INDICES = 5  # 1.0, 1.3, 1/1.3, 1.5, 1/1.5


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("serve_y_check") / "serve_y_check")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-w", "-o", exe, os.path.join(REPO, "tests", "serve_y_check.c"), "-lm",
                    "-lpthread"], check=True, timeout=300)
    p = subprocess.run([exe, str(PER_INDEX)], capture_output=True, text=True, timeout=600)
    print(p.returncode, p.stdout.strip(), p.stderr.strip())
    return p.returncode, json.loads(p.stdout)


def test_no_output_bit_differs(counts):
    """Every case's new origin, new direction and consumed-uniform flag carry the general body's bits, over both faces
    and both sides in equal shares and all eight families; the draws reach both forms and all three outcomes (total
    reflection, reflection by the draw, refraction), directions with zero components, and cos_theta = 1."""
    rc, r = counts
    n = PER_INDEX * INDICES
    assert r["cases"] == n and r["per_index"] == PER_INDEX
    assert r["wrong"] == 0 and rc == 0
    assert r["families"] == [n // 8] * 8
    assert [r["up_face4"], r["up_face5"], r["down_face4"], r["down_face5"]] == [n // 4] * 4
    assert r["reduced"] + r["fell_back"] == n and r["reduced"] > n // 4 and r["fell_back"] > n // 8
    assert min(r["tir"], r["reflected"], r["refracted"]) > n // 20
    assert r["zero_components_out"] > n // 20 and r["cos_at_or_above_one"] > n // 20


def test_controls_are_reported(counts):
    """The two controls, printed by the fixture and not asserted on: `control_no_zero_rule` (the reduced form on every
    lane) and `control_no_fmin` (cos_theta without the minimum).  Only their presence is checked."""
    _, r = counts
    print("control_no_zero_rule", r["control_no_zero_rule"], "control_no_fmin", r["control_no_fmin"])
    assert r["control_no_zero_rule"] >= 0 and r["control_no_fmin"] >= 0
