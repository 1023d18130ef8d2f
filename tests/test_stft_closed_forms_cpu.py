"""stftutil.py on the CPU: the closed forms against the float64 oracle, the
position and bin sets, and what the checkers can see.

  * for every family at N = 16, 1024 and 8192 the closed forms agree with
    oracle.np_stft_mag to 1e-12 of the frame's scale, and the reference passes
    every checker with no case left out;
  * the sets are sorted, unique, inside range and hold the seams of the
    kernels' index splits;
  * sensitivity: the checkers reject four deliberately wrong float64 models of
    an STFT (one window sample, two exchanged bins, one twiddle of the real
    split, frames read a sample late), each of which moves one index only;
  * the gap this closes: the parity suite's own white-noise check accepts the
    wrong window sample.
"""
import functools

import numpy as np
import pytest

import oracle
import stftutil as su
from test_gpu_parity import PEAK_REL_TOL, peak_rel_err, rnd

WINDOWS = [oracle.WIN_HANN, oracle.WIN_HAMMING, oracle.WIN_RECT]
SIZES = [16, 1024, 8192]
A1, A2 = 1.0, -0.625


def test_bars_are_the_projects():
    assert su.PEAK_REL_TOL == PEAK_REL_TOL == 1e-6 and su.ABS_FLOOR == 2.0 ** -61


# ---------------------------------------------------------------------------
# closed forms against the oracle
# ---------------------------------------------------------------------------
def rel(a, b, scale):
    return float(np.max(np.abs(a - b) / scale[:, None]))


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("N", SIZES)
def test_closed_forms_match_oracle(N, window):
    K = N // 2 + 1
    pos, pairs, bins = su.impulse_positions(N), su.impulse_pairs(N), su.tone_bins(N)
    for amp in (1.0, -0.75):
        x = su.impulse_frames(N, pos, amp)
        ref = oracle.np_stft_mag(x, N, N, window, K)
        assert ref.shape == (pos.size, K)
        got = su.impulse_mag(N, K, window, pos, amp)
        assert rel(got, ref, np.full(pos.size, abs(amp) / np.sqrt(N))) <= 1e-12
        assert su.check_impulses(ref, N, pos, amp, window) <= 1e-5
        assert su.check_frames(ref, got) <= 1e-5
    x = su.pair_frames(N, pairs, A1, A2)
    ref = oracle.np_stft_mag(x, N, N, window, K)
    assert ref.shape == (pairs.shape[0], K)
    assert rel(su.pair_mag(N, K, window, pairs, A1, A2), ref, np.full(pairs.shape[0], 1 / np.sqrt(N))) <= 1e-12
    assert su.check_pairs(ref, N, pairs, A1, A2, window) <= 1e-5
    x = su.tone_frames(N, bins)
    assert x.dtype == np.float32
    ref = su.tone_mag(N, K, window, x)
    assert ref.shape == (bins.size, K)
    assert su.check_tones(ref, ref, bins) == 0.0
    # a bin-centred tone: its own bin holds the peak (bins 0 and N/2 are real: twice the share)
    if window == oracle.WIN_RECT:
        peak = 0.5 * np.sqrt(N) / 2
        inner = (bins > 0) & (bins < N // 2)
        assert np.allclose(ref[np.arange(bins.size), bins][inner], peak, rtol=1e-6)
        assert np.array_equal(np.argmax(ref, axis=1)[inner], bins[inner])


@pytest.mark.parametrize("N", [1024, 8192])
def test_closed_forms_full_spectrum_and_stride(N):
    """K = N (the mirror path's shape) and a hop of N + 1 (the H = 8193 layout)"""
    pairs = su.impulse_pairs(N)
    x = su.pair_frames(N, pairs, A1, A2, hop=N + 1)
    assert x.size == (pairs.shape[0] - 1) * (N + 1) + N
    ref = oracle.np_stft_mag(x, N, N + 1, oracle.WIN_HAMMING, N)
    got = su.pair_mag(N, N, oracle.WIN_HAMMING, pairs, A1, A2)
    assert rel(got, ref, np.full(pairs.shape[0], 1 / np.sqrt(N))) <= 1e-12
    assert np.allclose(got[:, 1:], got[:, :0:-1], rtol=0, atol=1e-15)     # mag[k] == mag[N - k]


# ---------------------------------------------------------------------------
# the sets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 8, 16, 64, 256, 1024, 2048, 4096, 8192])
def test_sets_sorted_unique_in_range(N):
    pos, bins, pairs = su.impulse_positions(N), su.tone_bins(N), su.impulse_pairs(N)
    for v, hi in ((pos, N - 1), (bins, N // 2)):
        assert v.dtype == np.int64 and v.ndim == 1 and v.size > 0
        assert np.all(np.diff(v) > 0) and v[0] >= 0 and v[-1] <= hi
    assert pairs.ndim == 2 and pairs.shape[1] == 2 and pairs.shape[0] >= 4
    assert np.all(pairs[:, 0] < pairs[:, 1]) and pairs.min() >= 0 and pairs.max() < N
    key = pairs[:, 0] * N + pairs[:, 1]
    assert np.all(np.diff(key) > 0)
    if N <= 1024:
        assert np.array_equal(pos, np.arange(N))
    assert {0, 1, N // 2 - 1, N // 2}.issubset(bins.tolist()) and 0 in pos and N - 1 in pos
    for p in [(0, 1), (0, N // 2), (1, N - 1), (N // 2 - 1, N // 2)]:
        if p[0] != p[1]:
            assert p in set(map(tuple, pairs.tolist())), p


def test_sets_hold_the_seams_8192():
    N = 8192
    pos, bins, pairs = set(su.impulse_positions(N).tolist()), set(su.tone_bins(N).tolist()), \
        set(map(tuple, su.impulse_pairs(N).tolist()))
    assert set(range(256)) <= pos and set(range(N - 256, N)) <= pos
    for b in range(64):                                   # n = 2 lane + parity + 128 b: lanes 0 and 63 of every b
        assert {128 * b, 128 * b + 1, 128 * b + 127} <= pos
    for p in range(14):
        assert {2 ** p - 1, 2 ** p, 2 ** p + 1} & set(range(N)) <= pos
    assert len(pos) <= 820                                # one call: about 800 frames, 26 MB
    # k = lane + 64 q: lane 0 / q = 0, the partners' fixed points 1024, 2048, 3072, and the last bins
    assert {0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 1023, 1024, 1025, 2047, 2048, 2049,
            3071, 3072, 3073, 4032, 4033, 4094, 4095, 4096} <= bins
    for lane in su.PAIR_LANES:
        assert (2 * lane, 2 * lane + 1) in pairs and (2 * lane + 1, 2 * lane + 129) in pairs
        assert (2 * lane, 2 * lane + 4096) in pairs
    assert len(pairs) >= 48


# ---------------------------------------------------------------------------
# sensitivity: float64 models of an N-point STFT through the real split,
# each wrong in one index
# ---------------------------------------------------------------------------
def model(x, N, window, K, w_scale=None, swap=None, bad_twiddle=None, late=0):
    """magnitudes [F, K] of hop-N frames of x: window, the N/2-point complex
    FFT of (even, odd) samples, X[k] = E[k] + W_N^k O[k].
    w_scale = (n, s): window sample n times s.  swap = k: bins k and N/2 - k
    exchanged.  bad_twiddle = k: W_N^k replaced by W_N^(k + 1).  late: frames
    start `late` samples late."""
    w = oracle.np_window(window, N).copy()
    if w_scale is not None:
        w[w_scale[0]] *= w_scale[1]
    F = x.size // N
    xp = np.concatenate([x.astype(np.float64), np.zeros(late)])
    fr = xp[late:late + F * N].reshape(F, N) * w
    h = N // 2
    Z = np.fft.fft(fr[:, 0::2] + 1j * fr[:, 1::2], axis=1)
    Zc = np.conj(Z[:, (-np.arange(h)) % h])
    E, O = (Z + Zc) / 2, (Z - Zc) / 2j
    tw = np.exp(-2j * np.pi * np.arange(h + 1) / N)
    if bad_twiddle is not None:
        tw[bad_twiddle] = np.exp(-2j * np.pi * (bad_twiddle + 1) / N)
    X = np.empty((F, h + 1), complex)
    X[:, :h] = E + tw[:h] * O
    X[:, h] = E[:, 0] - O[:, 0]
    m = np.abs(X) / np.sqrt(N)
    if swap is not None:
        m[:, [swap, h - swap]] = m[:, [h - swap, swap]]
    return m[:, :K]


@functools.lru_cache(None)
def family(N, name):
    """(signal, check(mag, window)) of one family at N"""
    if name == "impulses":
        pos = su.impulse_positions(N)
        return su.impulse_frames(N, pos, 1.0), lambda m, win: su.check_impulses(m, N, pos, 1.0, win)
    if name == "pairs":
        pairs = su.impulse_pairs(N)
        return su.pair_frames(N, pairs, A1, A2), lambda m, win: su.check_pairs(m, N, pairs, A1, A2, win)
    bins = su.tone_bins(N)
    x = su.tone_frames(N, bins)
    return x, lambda m, win: su.check_tones(m, su.tone_mag(N, N // 2 + 1, win, x), bins)


def verdict(N, name, window, **wrong):
    """True when the family's checker accepts the model"""
    x, check = family(N, name)
    try:
        check(model(x, N, window, N // 2 + 1, **wrong), window)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("name", ["impulses", "pairs", "tones"])
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("N", SIZES)
def test_right_model_passes(N, window, name):
    assert verdict(N, name, window)


@pytest.mark.parametrize("window", WINDOWS)
def test_a_one_window_sample_centre(window):
    """w[n] (1 + 2e-5) at a centre sample: 20 bars for the impulse that sits on it"""
    for n in (4096, 4095, 4097):
        assert not verdict(8192, "impulses", window, w_scale=(n, 1 + 2e-5))


@pytest.mark.parametrize("window", [oracle.WIN_HAMMING, oracle.WIN_RECT])
def test_a_one_window_sample_n1(window):
    """... and at n = 1.  (Hann's w[1] is 1.5e-7 of the window's peak: 2e-5 of it
    is far below float32's resolution of the frame, and no bar can see it.)"""
    assert not verdict(8192, "impulses", window, w_scale=(1, 1 + 2e-5))
    assert oracle.np_window(oracle.WIN_HANN, 8192)[1] < 2e-7


def test_a_noise_check_accepts_the_wrong_window_sample():
    """The gap this file closes.  test_gpu_parity.test_stft_8192_vs_f64's own
    input (white noise, its shape and seed) and its own check, peak_rel_err <=
    1e-6, accept the window with its centre sample off by 2e-5: one sample of
    8192 moves a noise frame by about 2e-7 of its peak.  The single impulse on
    that sample rejects it (test_a_one_window_sample_centre)."""
    N, H, K = 8192, 8192, 4097
    x = rnd((2, 8192 * 3 + 1234), 21)
    for window in (oracle.WIN_HANN, oracle.WIN_HAMMING):
        for c in range(2):
            ref = oracle.np_stft_mag(x[c], N, H, window, K)
            wrong = model(x[c][:3 * N], N, window, K, w_scale=(4096, 1 + 2e-5))
            assert wrong.shape == ref.shape
            err = peak_rel_err(wrong, ref)
            print("noise check: wrong window sample, peak-relative error", err)
            assert 1e-8 < err <= PEAK_REL_TOL
            assert peak_rel_err(model(x[c][:3 * N], N, window, K), ref) <= 1e-12


@pytest.mark.parametrize("N,k", [(8192, 1), (8192, 700), (8192, 2047), (1024, 3), (16, 1)])
def test_b_exchanged_bins(N, k):
    """bins k and N/2 - k exchanged: flat spectra cannot see it, interfering impulses and the tone at k do"""
    for window in (oracle.WIN_HANN, oracle.WIN_RECT):
        assert verdict(N, "impulses", window, swap=k)
        assert not verdict(N, "pairs", window, swap=k)
    if k in su.tone_bins(N):
        assert not verdict(N, "tones", oracle.WIN_HANN, swap=k)


@pytest.mark.parametrize("N,k", [(8192, 1), (8192, 64), (8192, 1024), (8192, 2999), (8192, 4095), (1024, 65), (16, 3)])
def test_c_one_split_twiddle(N, k):
    """W_N^k -> W_N^(k + 1) for one k: a phase error.  A single impulse is all
    even or all odd part, so its magnitude does not depend on the twiddle's
    phase; a pair (2l, 2l + 1) has both parts and does."""
    for window in (oracle.WIN_HANN, oracle.WIN_RECT):
        assert verdict(N, "impulses", window, bad_twiddle=k)
        assert not verdict(N, "pairs", window, bad_twiddle=k)
    if k in su.tone_bins(N):
        assert not verdict(N, "tones", oracle.WIN_HANN, bad_twiddle=k)


@pytest.mark.parametrize("name", ["impulses", "pairs", "tones"])
@pytest.mark.parametrize("N", SIZES)
def test_d_frames_one_sample_late(N, name):
    for window in WINDOWS:
        assert not verdict(N, name, window, late=1)


# ---------------------------------------------------------------------------
# why impulses are not scaled by their own frame's peak
# ---------------------------------------------------------------------------
def test_computed_window_model():
    """stft_pk.hpp's computed window restated in float32 numpy (rounded
    products, no fused multiply-add): w(n) = (v S_b + wa) - u C_b with the
    lane's base angle in (u, v), n = 2 lane + parity + 128 b.  Its absolute
    error is about 1.2e-7 of the window's peak, many times w(n) itself near a
    Hann window's ends: check_sparse's scale is the window's peak, and its
    1e-6 leaves room for rounding only."""
    F32 = np.float32
    th, sc = 2 * np.pi / 8191, 0.5 / np.sqrt(8192)
    lane, b = np.arange(64), np.arange(64)
    Cb, Sb = np.cos(th * 128 * b).astype(F32), np.sin(th * 128 * b).astype(F32)
    for (a_, b_) in ((0.5, 0.5), (0.54, 0.46)):
        wa, wb = F32(a_ * sc), F32(b_ * sc)
        w = np.empty(8192, F32)
        for par in (0, 1):
            u = wb * np.cos(th * (2 * lane + par)).astype(F32)
            v = wb * np.sin(th * (2 * lane + par)).astype(F32)
            for q in b:
                w[2 * lane + par + 128 * q] = (v * Sb[q] + wa) - u * Cb[q]
        ref = (a_ - b_ * np.cos(th * np.arange(8192))) * sc
        err = np.abs(w - ref).max() / ref.max()
        print("computed window model: max error / max(w)", err)
        assert 2e-8 < err < 1.5e-7
        if a_ == 0.5:
            assert np.abs(w[1] - ref[1]) > 0.01 * ref[1]      # a frame's own peak cannot be the scale there
