"""The float64 numpy model of dsp_resample (include/dspbench/dspbench.h): h
evaluated directly per output with np.i0, nothing shared with the library."""
from math import gcd

import numpy as np

DEFAULTS = dict(zeros=64, beta=14.769656459379492, rolloff=0.9475937167399596)


def plan(sr_in, sr_out, L=0, zeros=64, beta=DEFAULTS["beta"], rolloff=DEFAULTS["rolloff"]):
    g = gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    rho = rolloff * min(1.0, up / down)
    W = zeros / rho
    half = int(np.ceil(W))
    return dict(up=up, down=down, rho=rho, W=W, half=half, taps=2 * half, beta=beta,
                Lout=(L * up + down - 1) // down)


def h(p, u):
    u = np.asarray(u, np.float64)
    inside = np.abs(u) < p["W"]
    r = np.where(inside, u / p["W"], 0.0)
    v = p["rho"] * np.sinc(p["rho"] * u) * np.i0(p["beta"] * np.sqrt(1.0 - r * r)) / np.i0(p["beta"])
    return np.where(inside, v, 0.0)


def table64(p):
    """table[phi][i] = h(half - 1 - i + phi / up) in float64."""
    i = np.arange(p["taps"], dtype=np.float64)
    phi = np.arange(p["up"], dtype=np.float64)[:, None]
    return h(p, (p["half"] - 1.0 - i)[None, :] + phi / p["up"])


def resample_f64(x, sr_in, sr_out, **spec):
    """y[m] = sum_i h(half - 1 - i + phi / up) x[n0 - half + 1 + i], x = 0 outside."""
    x = np.asarray(x, np.float64)
    p = plan(sr_in, sr_out, x.size, **spec)
    half, taps = p["half"], p["taps"]
    xp = np.concatenate([np.zeros(half), x, np.zeros(half + 1)])   # xp[k] = x[k - half]
    m = np.arange(p["Lout"], dtype=np.int64)
    q = m * p["down"]
    n0, phi = q // p["up"], q % p["up"]
    i = np.arange(taps, dtype=np.int64)
    y = np.empty(p["Lout"])
    step = max(1, (1 << 22) // taps)
    for a in range(0, p["Lout"], step):
        b = min(p["Lout"], a + step)
        u = (half - 1 - i)[None, :] + (phi[a:b, None] / p["up"])
        y[a:b] = np.sum(h(p, u) * xp[(n0[a:b, None] + 1 + i[None, :])], axis=1)
    return y


def inputs(seed, C, L):
    return np.random.default_rng(seed).uniform(-1, 1, (C, L)).astype(np.float32)
