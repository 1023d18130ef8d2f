#!/usr/bin/env python3
"""MODEL32: dsp_limiter's definition as a serial float32 chain on the CPU --
every product, quotient, difference and max rounded to float32, the release
one multiplication by rho per sample, the attack sum k = 0..A in order.  It is
the float32 yardstick behind LIM_TOL (tests/limiterutil.py): how far plain
float32 arithmetic lands from the float64 model.

  limiter_model.py tol      the worst |g32 - g64| over the GPU tests' cases
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import limiterutil as lu  # noqa: E402

f32 = np.float32


def gain32(p, c, A, tau):
    """g[n] in float32 from a float32 detector row."""
    p = np.asarray(p, f32)
    c = f32(c)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(p > c, f32(1.0) - c / np.where(p > c, p, f32(1.0)), f32(0.0)).astype(f32)
    h = lu.hold(a, A)
    r = lu.rho(tau)
    e = np.empty_like(h)
    prev = f32(0.0)
    for n in range(h.size):
        prev = e[n] = max(h[n], f32(r * prev))
    w = lu.window(A)
    s = np.zeros_like(e)
    for k in range(min(A + 1, e.size)):
        s[k:] = s[k:] + w[k] * e[:e.size - k]  # float32 arrays: each product and each sum rounds
    return f32(1.0) - s


def detector32(x, sr, true_peak):
    """p[n] of one link group in float32: the polyphase sums over the float32
    table, products and sums rounded one by one, i = 0..Tp - 1 in order."""
    x = np.atleast_2d(np.asarray(x, f32))
    p = np.abs(x).max(axis=0)
    ovs = lu.oversample(sr) if true_peak else 1
    if ovs > 1 and x.shape[1]:
        rp = lu.resampleutil.plan(sr, sr * ovs)
        T = lu.resampleutil.table64(rp).astype(f32)
        half, n = rp["half"], x.shape[1]
        for ch in range(x.shape[0]):
            xp = np.concatenate([np.zeros(half - 1, f32), x[ch], np.zeros(half, f32)])
            for phi in range(ovs):
                acc = np.zeros(n, f32)
                for i in range(rp["taps"]):
                    acc = acc + T[phi, i] * xp[i:i + n]
                p = np.maximum(p, np.abs(acc))
    return p


def limiter32(x, sr, c, A, tau, true_peak=False, linked=True):
    """g32 [groups, L]."""
    x = np.atleast_2d(np.asarray(x, f32))
    groups = [list(range(x.shape[0]))] if linked else [[ch] for ch in range(x.shape[0])]
    return np.stack([gain32(detector32(x[rows], sr, true_peak), c, A, tau) for rows in groups])


def tol():
    worst, where = 0.0, None
    for k in lu.CASES:
        x = lu.case_input(k)
        args = (x, k["sr"], lu.CEILING, k["A"], k["tau"], k["true_peak"], k["linked"])
        g64 = lu.limiter64(*args)[0]
        err = float(np.max(np.abs(limiter32(*args).astype(np.float64) - g64)))
        if err > worst:
            worst, where = err, lu.case_id(k)
    print(f"MODEL32 worst |g32 - g64| = {worst:.3e} at {where} over {len(lu.CASES)} cases")
    return worst


if __name__ == "__main__":
    if sys.argv[1:] == ["tol"]:
        tol()
    else:
        sys.exit(__doc__)
