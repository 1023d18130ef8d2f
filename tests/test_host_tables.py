"""csrc/host_tables.cpp: the float64 host maths behind the device tables,
compiled with g++ alone (no HIP) into tests/sanitize/host_tables_check.cpp and
checked against the definitions of what the tables hold; once more under
AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone host program).
"""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "dsp-bench_amd", "csrc")


def run_check(tmp, san):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host tables alone"
    exe = str(tmp / ("host_tables_check" + ("_san" if san else "")))
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O2"]
    r = subprocess.run([gxx, "-std=c++17", "-Wall", *flags, f"-I{CSRC}", f"{HERE}/sanitize/host_tables_check.cpp",
                        f"{CSRC}/host_tables.cpp", "-o", exe], capture_output=True, text=True, timeout=300)
    if san and r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("the compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return [ln.split() for ln in r.stdout.splitlines()]


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def figures(request, tmp_path_factory):
    return run_check(tmp_path_factory.mktemp("host_tables"), request.param)


def value(figures, name):
    return float(next(f[1] for f in figures if f[0] == name))


def test_taps_spectrum_is_the_dft(figures):
    """Against a direct O(n^2) float64 DFT at n = 64: both sum 23 products of
    magnitude <= peak with float64 roundings, 1e-13 of the peak is generous."""
    assert value(figures, "spectrum_peak") > 1.0
    assert value(figures, "spectrum_max_diff") <= 1e-13 * value(figures, "spectrum_peak")


def test_biquad_tables_are_powers_of_the_transition(figures):
    """One section with poles 0.9 e^(+-0.3i) (coefficients 1, 0.5, 0.25,
    -1.8 cos 0.3, 0.81 as floats): Q[l] = A^(32 l) and P[k] = A^(2048 k) in
    closed form, each block within 1e-6 of its largest entry (float storage of
    float64 products: 6e-8 plus the products' own roundings)."""
    assert value(figures, "biquad_coef_ok") == 1
    assert value(figures, "biquad_Q_rel_err") <= 1e-6
    assert value(figures, "biquad_P_rel_err") <= 1e-6
    # ||A^(2048 k)|| ~ 0.9^(2048 k) is far below 2^-48 from k = 1 on: only the tile itself counts
    assert value(figures, "biquad_W") == 1


def ramp_is_exact(gain, step, B):
    """IR_test's recurrence `g -= step` in float64 from the float parameters
    equals the correctly rounded gain - i step (one fma) at every i < B."""
    if B > 1 << 16:
        return False  # the host check is bounded: larger blocks build the table
    g0, s = np.float64(np.float32(gain)), np.float64(np.float32(step))
    g = g0
    for i in range(B):
        if float(Fraction(float(g0)) - i * Fraction(float(s))) != float(g):
            return False
        g = g - s
    return True


def test_ramp_closed_form_matches_the_recurrence(figures):
    ramps = [f for f in figures if f[0] == "ramp"]
    assert len(ramps) == 5
    for _, gain, step, B, got in ramps:
        assert bool(int(got)) == ramp_is_exact(float(gain), float(step), int(B)), (gain, step, B)
    # the headline parameters (gain 0.9, step 0.002, B = 512): whatever the definition gives
    assert ramps[0][1:4] == ["0.899999976", "0.00200000009", "512"]
