"""Structured STFT / FFT inputs whose spectra are known in closed form, and
the checkers that compare a kernel's output with them (numpy only; checked on
the CPU by test_stft_closed_forms_cpu.py, used by test_gpu_stft_closed_forms.py).

White noise puts about 1/sqrt(N) of every sample, window value and twiddle
into every bin, so a defect confined to one index passes a peak-relative
bar.  Here one frame is one case: a single impulse looks at one window
sample, two impulses interfere and so look at twiddle phase, a bin-centred
tone looks at one output bin.

Index splits the sets follow (stft_pk.hpp): sample n = 2 lane + parity + 128 b,
bin k = lane + 64 q with partners 4096 - k and 2048 +- k.

Bars.  check_frames is the project's bar: per frame max|m - ref| <=
PEAK_REL_TOL * max(ref) + 2^-61 (test_gpu_parity, test_gpu_edge_values).
A frame of one or two impulses cannot be scaled by its own peak: near a Hann
window's ends that peak is 1e-7 of the window's or zero, while a float32
window a - b cos(theta n) carries an absolute rounding error of about 1e-7 of
its maximum (test_stft_closed_forms_cpu.test_computed_window_model).  So
check_sparse scales the same PEAK_REL_TOL by the largest magnitude impulses
of those amplitudes can produce, sum|a| max(w) / sqrt(N).
"""
import numpy as np

import oracle

PEAK_REL_TOL = 1e-6            # test_gpu_parity.PEAK_REL_TOL
ABS_FLOOR = 2.0 ** -61         # test_gpu_edge_values.ABS_FLOOR
SEED = 8192


# ---------------------------------------------------------------------------
# signal builders: frame f of a hop-`hop` call (default N) is case f
# ---------------------------------------------------------------------------
def _signal(N, F, hop):
    hop = N if hop is None else hop
    assert hop >= N and F > 0
    return np.zeros((F - 1) * hop + N, np.float32), np.arange(F, dtype=np.int64) * hop


def impulse_frames(N, positions, amp, hop=None):
    """amp at f * hop + positions[f]"""
    positions = np.asarray(positions, np.int64)
    x, base = _signal(N, positions.size, hop)
    x[base + positions] = amp
    return x


def pair_frames(N, pairs, a1, a2, hop=None):
    """a1 at pairs[f][0] and a2 at pairs[f][1] of frame f"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    assert np.all(pairs[:, 0] != pairs[:, 1])
    x, base = _signal(N, pairs.shape[0], hop)
    x[base + pairs[:, 0]] = a1
    x[base + pairs[:, 1]] = a2
    return x


def tone_frames(N, bins, amp=0.5, phase=0.3, hop=None):
    """amp cos(2 pi k n / N + phase), rounded to float32, in frame f for k = bins[f]"""
    bins = np.asarray(bins, np.int64)
    x, base = _signal(N, bins.size, hop)
    n = np.arange(N, dtype=np.int64)
    ang = 2.0 * np.pi * ((bins[:, None] * n[None, :]) % N) / N + phase
    x[base[:, None] + n[None, :]] = (amp * np.cos(ang)).astype(np.float32)
    return x


# ---------------------------------------------------------------------------
# position and bin sets
# ---------------------------------------------------------------------------
def _clip_unique(v, lo, hi):
    v = np.asarray(sorted(set(int(i) for i in v)), np.int64)
    return v[(v >= lo) & (v <= hi)]


def impulse_positions(N):
    """every n for N <= 1024; above that both ends (256 samples each), the
    first two and the last sample of every block of 128, the neighbours of
    every power of two, and 64 seeded draws"""
    if N <= 1024:
        return np.arange(N, dtype=np.int64)
    v = list(range(256)) + list(range(N - 256, N))
    for b in range(N // 128):
        v += [128 * b, 128 * b + 1, 128 * b + 127]
    p = 1
    while p <= N:
        v += [p - 1, p, p + 1]
        p *= 2
    v += list(np.random.default_rng(SEED + N).integers(0, N, 64))
    return _clip_unique(v, 0, N - 1)


def tone_bins(N):
    h = N // 2
    v = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, h - 64, h - 63, h - 2, h - 1, h]
    for c in (N // 8, N // 4, 3 * N // 8):
        v += [c - 1, c, c + 1]
    v += list(np.random.default_rng(SEED + N + 1).integers(0, h + 1, 32))
    return _clip_unique(v, 0, h)


PAIR_LANES = (0, 1, 31, 32, 63)


def impulse_pairs(N):
    """[P, 2], j1 < j2, sorted and unique"""
    h = N // 2
    v = [(0, 1), (0, h), (1, N - 1), (h - 1, h)]
    for lane in PAIR_LANES:
        v += [(2 * lane, 2 * lane + 1), (2 * lane + 128 * (N // 256), 2 * lane + 1 + 128 * (N // 256))]
        v += [(2 * lane + 1, 2 * lane + 1 + 128), (2 * lane, 2 * lane + 128 * (N // 128 - 1))]
        v += [(2 * lane, 2 * lane + h), (2 * lane + 1, 2 * lane + 1 + h)]
    rng = np.random.default_rng(SEED + N + 2)
    for _ in range(32):
        v.append(tuple(int(i) for i in rng.integers(0, N, 2)))
    s = sorted(set((min(a, b), max(a, b)) for a, b in v if a != b and 0 <= min(a, b) and max(a, b) < N))
    return np.asarray(s, np.int64).reshape(-1, 2)


# ---------------------------------------------------------------------------
# closed forms, float64
# ---------------------------------------------------------------------------
def sparse_cases(positions, amps):
    """(J [F, M], A [F, M]) of F frames holding impulse m at J[f, m] with amplitude A[f, m]"""
    J = np.asarray(positions, np.int64)
    J = J.reshape(J.shape[0], -1)
    A = np.broadcast_to(np.asarray(amps, np.float64), J.shape)
    return J, np.array(A)


def sparse_mag(N, K, window, J, A):
    """|sum_m A[f, m] w[J[f, m]] exp(-2 i pi k J[f, m] / N)| / sqrt(N) for k < K: [F, K]"""
    w = oracle.np_window(window, N)
    tab = np.exp(-2j * np.pi * np.arange(N) / N)
    k = np.arange(K, dtype=np.int64)
    out = np.empty((J.shape[0], K))
    for f0 in range(0, J.shape[0], 64):
        j, a = J[f0:f0 + 64], A[f0:f0 + 64]
        z = np.zeros((j.shape[0], K), complex)
        for m in range(j.shape[1]):
            z += (a[:, m] * w[j[:, m]])[:, None] * tab[(j[:, m, None] * k[None, :]) % N]
        out[f0:f0 + 64] = np.abs(z) / np.sqrt(N)
    return out


def impulse_mag(N, K, window, positions, amp):
    """every bin of frame f equals |amp| w[positions[f]] / sqrt(N)"""
    w = oracle.np_window(window, N)
    return np.repeat((abs(amp) * w[np.asarray(positions, np.int64)] / np.sqrt(N))[:, None], K, axis=1)


def pair_mag(N, K, window, pairs, a1, a2):
    """|a1 w[j1] + a2 w[j2] exp(-2 i pi k (j2 - j1) / N)| / sqrt(N)"""
    return sparse_mag(N, K, window, *sparse_cases(pairs, [a1, a2]))


def tone_mag(N, K, window, x, hop=None):
    """tones have no closed form of their own: the float64 STFT of the float32 signal"""
    return oracle.np_stft_mag(x, N, N if hop is None else hop, window, K)


# ---------------------------------------------------------------------------
# checkers: print the worst case, name the frame's case when they fail;
# return the worst error in units of the bar
# ---------------------------------------------------------------------------
def _check(mag, ref, bar, names, what):
    mag, ref = np.asarray(mag, np.float64), np.asarray(ref, np.float64)
    assert mag.shape == ref.shape and mag.ndim == 2, (what, mag.shape, ref.shape)
    assert np.isfinite(mag).all(), what
    bar = np.broadcast_to(np.asarray(bar, np.float64), (mag.shape[0],))
    err = np.abs(mag - ref)
    k = np.argmax(err, axis=1)
    e = err[np.arange(err.shape[0]), k]
    ratio = e / bar
    f = int(np.argmax(ratio))
    name = names[f] if names is not None else f
    msg = (f"{what}: worst {ratio[f]:.3f} of the bar at frame {f} (case {name}), bin {int(k[f])}: "
           f"got {mag[f, k[f]]:.9e} want {ref[f, k[f]]:.9e} err {e[f]:.3e} bar {bar[f]:.3e}; "
           f"{int(np.sum(ratio > 1))} of {ratio.size} frames over")
    print(msg)
    assert ratio[f] <= 1.0, msg
    return float(ratio[f])


def check_frames(mag, ref, names=None, what="frames", peak=None):
    """the project's bar: per frame max|m - ref| <= PEAK_REL_TOL peak + 2^-61.
    peak [F]: the frame's peak over all its bins, for a ref that holds only the
    first K of them (a tone above bin K leaves them near zero); default max(ref)."""
    ref = np.asarray(ref, np.float64)
    peak = ref.max(axis=1) if peak is None else np.asarray(peak, np.float64)
    assert np.all(peak >= ref.max(axis=1))
    return _check(mag, ref, PEAK_REL_TOL * peak + ABS_FLOOR, names, what)


def sparse_scale(N, window, A):
    """the largest magnitude impulses of amplitudes A[f, :] can produce"""
    return np.abs(np.asarray(A, np.float64)).reshape(len(A), -1).sum(axis=1) * oracle.np_window(window, N).max() / np.sqrt(N)


def check_sparse(mag, N, J, A, window, names=None, what="sparse"):
    """|m[f, k] - closed form| <= PEAK_REL_TOL sum_m |A[f, m]| max(w) / sqrt(N), every bin"""
    ref = sparse_mag(N, np.shape(mag)[1], window, J, A)
    return _check(mag, ref, PEAK_REL_TOL * sparse_scale(N, window, A), names, what)


def check_impulses(mag, N, positions, amp, window, what="impulses"):
    """|m[f, k] - |amp| w[j_f] / sqrt(N)| <= PEAK_REL_TOL |amp| max(w) / sqrt(N), every bin"""
    positions = np.asarray(positions, np.int64)
    ref = impulse_mag(N, np.shape(mag)[1], window, positions, amp)
    bar = PEAK_REL_TOL * abs(amp) * oracle.np_window(window, N).max() / np.sqrt(N)
    return _check(mag, ref, bar, [f"j={j}" for j in positions], what)


def check_pairs(mag, N, pairs, a1, a2, window, what="pairs"):
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    J, A = sparse_cases(pairs, [a1, a2])
    return check_sparse(mag, N, J, A, window, [f"j=({a},{b})" for a, b in pairs], what)


def check_tones(mag, ref, bins, what="tones", peak=None):
    return check_frames(mag, ref, [f"k={k}" for k in bins], what, peak)
