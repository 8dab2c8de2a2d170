"""The serve body written out for a y face (rt_device.h serve_y) against the general device functions it replaces —
hit_record, unit_fast, shade_dielectric — on the GPU, side by side on 2^20 adversarial cases (tools/servecheck.hip;
the families of tests/serve_y_check.c): the same bits in the new origin, the new direction and the RNG state.  The
only place where the lanes serve_y hands back (zero and tiny components) are certain to occur on the device: a render
does not produce exact zeros."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "shirley-raytracing-rs_amd", "bin",
                   "servecheck")


def test_serve_y_is_bit_identical_to_the_general_body():
    assert os.path.exists(BIN), "bin/servecheck not built (make -C shirley-raytracing-rs_amd)"
    r = subprocess.run([BIN, "20"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"servecheck: (\d+) cases, (\d+) differ, (\d+) by serve_y, (\d+) handed back, (\d+) totally reflected, "
                 r"(\d+) reflected, (\d+) refracted", r.stdout)
    assert m, r.stdout
    cases, differ, by_y, back, tir, refl, refr = map(int, m.groups())
    assert cases == 1 << 20 and differ == 0 and by_y + back == cases and tir + refl + refr == by_y
    # every branch is exercised: both forms, and all three outcomes of the reduced one
    assert by_y > cases // 4 and back > cases // 8 and min(tir, refl, refr) > cases // 100
