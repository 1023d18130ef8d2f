"""The float64 numpy model of dsp_limiter (include/dspbench/dspbench.h), written
from the definition: detector, needed attenuation, look-ahead hold, release,
attack smoothing, gain.  Nothing shared with the library: it takes the float32
inputs, computes its own window and rho in float64 and uses resampleutil's h
for the oversampled detector.  Also the cases and inputs the GPU tests and
tools/limiter_model.py run."""
import numpy as np

import resampleutil

TILE = 2048

# |g - g64| <= LIM_TOL, |y - x g64| <= LIM_TOL |x| + one ulp: 4 x the larger of
# the two worst cases of max |g - g64| over CASES (the convention of CONV_TOL,
# RESAMPLE_TOL and LOUD_TOL):
#   MODEL32 (tools/limiter_model.py tol, on the CPU)   1.735e-06  (A = 1024, L = 20000, tau = 4800)
#   the GPU's own worst case (MI355X, test_model)      1.482e-06  (A = 1024, L = 2047, tau = 4800)
# Both are a few ulps of 1: the attack sum of up to 1025 float32 terms dominates.
MODEL32_WORST = 1.735e-6
GPU_WORST = 1.482e-6
LIM_TOL = 4.0 * max(MODEL32_WORST, GPU_WORST)


def oversample(sr):
    return 4 if sr < 88200 else 2 if sr < 176400 else 1


def window64(A):
    v = np.sin(np.pi * (np.arange(A + 1, dtype=np.float64) + 1.0) / (A + 2.0)) ** 2
    return v / v.sum()


def window(A):
    """w as the definition rounds it: once, to float32."""
    return window64(A).astype(np.float32)


def rho(tau):
    return np.float32(0.0) if tau == 0 else np.float32(np.exp(-1.0 / float(tau)))


def detector64(x, sr, true_peak):
    """p[n] of one link group x [C, L] in float64."""
    x = np.atleast_2d(np.asarray(x, np.float32)).astype(np.float64)
    p = np.abs(x).max(axis=0)
    ovs = oversample(sr) if true_peak else 1
    if ovs > 1 and x.shape[1]:
        rp = resampleutil.plan(sr, sr * ovs)
        T = resampleutil.table64(rp)  # [ovs, taps]
        half = rp["half"]
        for c in range(x.shape[0]):
            xp = np.concatenate([np.zeros(half - 1), x[c], np.zeros(half)])  # xp[k] = x[k - half + 1]
            for phi in range(ovs):
                p = np.maximum(p, np.abs(np.correlate(xp, T[phi], "valid")[:x.shape[1]]))
    return p


def hold(a, A):
    """h[n] = max a[n .. n + A], a = 0 past the end."""
    ap = np.concatenate([a, np.zeros(A, a.dtype)])
    return np.lib.stride_tricks.sliding_window_view(ap, A + 1).max(axis=1) if a.size else a


def gain64(p, c, A, tau):
    """g[n] in float64 from a detector row: steps 2-6 with the definition's
    float32 constants (c, rho, w) taken to float64."""
    c = float(np.float32(c))
    p = np.asarray(p, np.float64)
    a = np.where(p > c, 1.0 - c / np.where(p > c, p, 1.0), 0.0)
    h = hold(a, A)
    r = float(rho(tau))
    e = np.empty_like(h)
    prev = 0.0
    for n in range(h.size):
        prev = e[n] = max(h[n], r * prev)
    w = window(A).astype(np.float64)
    s = np.convolve(e, w)[:e.size] if e.size else e
    return 1.0 - s


def limiter64(x, sr, c, A, tau, true_peak=False, linked=True):
    """(g64 [groups, L], y64 [C, L], p64 [groups, L]) of the whole call; y64 = x g64 clamped."""
    x = np.atleast_2d(np.asarray(x, np.float32))
    groups = [list(range(x.shape[0]))] if linked else [[ch] for ch in range(x.shape[0])]
    c64 = float(np.float32(c))
    g, p, y = [], [], np.empty(x.shape, np.float64)
    for rows in groups:
        p.append(detector64(x[rows], sr, true_peak))
        g.append(gain64(p[-1], c, A, tau))
        y[rows] = np.clip(x[rows].astype(np.float64) * g[-1], -c64, c64)
    return np.stack(g), y, np.stack(p)


def inputs(seed, C, L, c, A):
    """Seeded noise at about 0.3 of the ceiling, plus isolated peaks of 2-8 x the
    ceiling at 0, 2047, 2048, L - 1 and at A + 1 apart (where the rows hold them)."""
    rng = np.random.default_rng(seed)
    x = (0.3 * c * rng.uniform(-1, 1, (C, L))).astype(np.float32)
    at = [0, 2047, 2048, L - 1, 700, 700 + A + 1, 3000, 3000 + A + 1, 3000 + 2 * (A + 1)]
    for j, n in enumerate(at):
        if 0 <= n < L:
            x[j % C, n] = np.float32(c * (2.0 + 6.0 * rng.uniform()) * (1 if j % 2 else -1))
    return x


def quiet(seed, C, L, c):
    """max |x| <= c, with samples at the ceiling itself."""
    x = (c * np.random.default_rng(seed).uniform(-1, 1, (C, L))).astype(np.float32)
    x = np.clip(x, -np.float32(c), np.float32(c))
    if L:
        x[0, 0] = np.float32(c)
        x[-1, -1] = -np.float32(c)
    return x


CEILING = float(np.float32(10.0 ** (-1.0 / 20.0)))
LOOKAHEADS = (0, 1, 63, 64, 1024)
RELEASES = (0, 64, 4800)
CHANNELS = (1, 2, 3, 17)
DETECTORS = ((False, 48000), (True, 48000), (True, 96000), (True, 192000))


def lengths(A):
    return [n for n in dict.fromkeys((1, A, A + 1, 2047, 2048, 2049, 2 * 2048 + A + 3, 20000)) if n > 0]


def _cases():
    """Every length of every lookahead, with the release, the channel count and
    the detector walking their lists so each value meets each lookahead; 17
    channels stay on rows of at most 2049 samples but for one extra case, and
    tau = 4800 at L = 20000 (a release carried across >= 3 tiles) runs at every
    lookahead."""
    out, k = [], 0
    for A in LOOKAHEADS:
        for L in lengths(A):
            tau = 4800 if L == 20000 else RELEASES[k % 3]
            C = CHANNELS[(k // 2) % 4]
            tp, sr = DETECTORS[(k + k // 8) % 4]
            if C == 17 and L > 2049:  # (17 channels on long rows: the extra cases below)
                C = 2
            out.append(dict(A=A, L=L, tau=tau, C=C, true_peak=tp, sr=sr, linked=(k % 5 != 4), seed=100 + k))
            k += 1
    # what the walk above may miss: each detector rate and 17 linked channels on rows of several tiles
    for j, (tp, sr) in enumerate(DETECTORS):
        out.append(dict(A=63 + j, L=2 * 2048 + 70, tau=RELEASES[j % 3], C=(17, 3, 2, 1)[j], true_peak=tp, sr=sr,
                        linked=True, seed=900 + j))
    return out


CASES = _cases()


def case_id(k):
    return "A{A}-L{L}-tau{tau}-C{C}-{d}{sr}-{l}".format(d="tp" if k["true_peak"] else "sp",
                                                         l="linked" if k["linked"] else "unlinked", **k)


def case_input(k):
    return inputs(k["seed"], k["C"], k["L"], CEILING, k["A"])
