#!/usr/bin/env python3
"""MODEL32 of the large real FFT and of dsp_deconvolve against float64, over
the GPU tests' own inputs (tests/deconvutil.py holds both models): the figures
behind FFT_TOL, DEC_TOL and RECOVERY_TOL.

  deconv_model.py tol [--big]   the worst e_fft, e_dec and the recovery error
                                (--big adds n = 2^24: a minute of numpy)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import deconvutil as du  # noqa: E402


def e_fft(x, n):
    X64 = du.rfft64(x, n)
    return float(np.max(np.abs(du.rfft32(x, n) - X64)) / np.max(np.abs(X64)))


def fft_worst(big):
    worst = (0.0, "")
    for n in du.FFT_NS:
        for name, x in du.fft_cases(n):
            worst = max(worst, (e_fft(x, n), f"{name} n={n}"))
            if name in ("noise", "decay"):  # the inverse of the float64 spectrum, relative to the row's peak
                X = du.rfft64(x, n)
                xp = np.zeros(n)
                xp[:x.size] = x
                e = float(np.max(np.abs(du.irfft32(X.astype(du.c64), n) - xp)) / np.max(np.abs(xp)))
                worst = max(worst, (e, f"inverse {name} n={n}"))
    if big:
        n = du.BIG_N
        worst = max(worst, (e_fft(du.noise(n, 1, n)[0], n), f"noise n={n}"))
    return worst


def dec_worst():
    worst = (0.0, "")
    for k in du.DEC_CASES:
        rec, ref = du.dec_case_input(k)
        h64 = du.deconv64(rec, ref, k["eps"], k["pre"], k["ir_len"])
        h32 = du.deconv32(rec, ref, k["eps"], k["pre"], k["ir_len"])
        scale = np.max(np.abs(du.deconv64(rec, ref, k["eps"], 0, None)))  # the whole response's peak
        worst = max(worst, (float(np.max(np.abs(h32 - h64)) / scale), k["name"]))
    return worst


def recovery():
    k = du.DEC_CASES[0]
    rec, ref = du.dec_case_input(k)
    h64 = du.deconv64(rec, ref, k["eps"], k["pre"], k["ir_len"])[0]
    h = np.zeros(h64.size)
    h[:1024] = du.bandpass_ir(L=1024)
    return float(np.max(np.abs(h64 - h)) / np.max(np.abs(h)))


def main():
    if len(sys.argv) < 2 or sys.argv[1] != "tol":
        sys.exit(__doc__)
    f, fname = fft_worst("--big" in sys.argv)
    print(f"e_fft  worst {f:.3e} ({fname})   FFT_TOL = 4 x = {4 * f:.3e}")
    e, ename = dec_worst()
    print(f"e_dec  worst {e:.3e} ({ename})   DEC_TOL = 4 x = {4 * e:.3e}")
    print(f"recovery (float64 model against the known h): {recovery():.3e}")


if __name__ == "__main__":
    main()
