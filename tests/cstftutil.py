"""Shapes, inputs, references and the tolerances of the dsp_stft / dsp_istft
tests (test_stft_cx_host.py, test_gpu_stft_cx.py).  The float64 references come
from tools/stft_model.py and are computed once per case.

STFT_TOL:  per frame max_k |X - X64| <= STFT_TOL max_k |X64|.
ISTFT_TOL: per row max_i |y - y64| / A[i] <= ISTFT_TOL max_f max |v_f| over the
           samples with den >= 2 floor; A is the noise gain sum |w| / den.
Each is 4 x the larger of two worst ratios measured over exactly CASES, the way
WELCH_TOL was set; the factor 4 covers inputs not in the list.
  float32 CPU model (tools/stft_model.py stft32 / istft32 against the float64
  models):                                        MODEL_RATIO_FWD / MODEL_RATIO_INV
  the GPU (dsp_stft / dsp_istft against them, MI355X): GPU_RATIO_FWD / GPU_RATIO_INV

The band the contract leaves open.  A sample whose exact den lies in
[floor / 2, 2 floor) may come out 0 or as the quotient.  With Hamming no sample
falls below floor at all.  With Hann the band cannot be made empty: where a
frame begins or ends with no other frame over it (both ends of the output, and
every frame edge at hop N) den follows w[j]^2 = (pi j / 8191)^4, j samples from
the edge; successive values differ by less than the band's factor 4 from j = 3
on, and the one wider gap (j = 2 to 3) lies below the least floor the call
accepts.  So envelope() names the band's samples -- at most three at a frame
edge, within 16 samples of it, asserted here -- and the tests accept for them
either outcome and nothing else: no sample is skipped.
"""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import stft_model as sm  # noqa: E402
import welchutil as wu  # noqa: E402

N, K = sm.N, sm.K
MAXCH = 16
FLOOR = 1e-10  # the calls' default

MODEL_RATIO_FWD = 2.09e-7
MODEL_RATIO_INV = 2.27e-7
GPU_RATIO_FWD = 2.63e-7
GPU_RATIO_INV = 2.58e-7
STFT_TOL = 4.0 * max(MODEL_RATIO_FWD, GPU_RATIO_FWD)
ISTFT_TOL = 4.0 * max(MODEL_RATIO_INV, GPU_RATIO_INV)

Case = namedtuple("Case", "F H C window signal fwd inv")

# (F, H, C): one frame; the four-wave block and one past it; hop N; rows 4 bytes
# off alignment (odd hop); a hop that is no multiple of anything; two channel
# groups at hop 1 (forward only); the smallest odd hop the inverse takes
SHAPES = [(1, 4096, 1), (4, 4096, 2), (5, 4096, 2), (3, 8192, 1), (5, 4095, 2), (6, 2730, 3), (9, 1, 17), (5, 513, 1)]
# inverse only: overlap 16; chunk + 1 at 16 rows (one group, and two); chunk + 1 at one row
INVERSE_SHAPES = [(17, 512, 1, None), (129, 512, 16, "hann"), (129, 1024, 17, "hamming"), (2049, 512, 1, "hann")]

CASES = [Case(F, H, C, w, s, True, H >= 512 and s == "noise")
         for (F, H, C) in SHAPES for w in ("hann", "hamming") for s in ("noise", "tones")]
CASES += [Case(F, H, C, w, "noise", False, True)
          for (F, H, C, only) in INVERSE_SHAPES for w in ("hann", "hamming") if only in (None, w)]
# the 16-row chunk seam under the other window too (appended: a case's seed is its index)
CASES += [Case(129, 512, 16, "hamming", "noise", False, True), Case(129, 1024, 17, "hann", "noise", False, True)]
FORWARD = [c for c in CASES if c.fwd]
INVERSE = [c for c in CASES if c.inv]
ROUND_TRIP = [c for c in FORWARD if c.H >= 512]


def case_id(c):
    return f"F{c.F}-H{c.H}-C{c.C}-{c.window}-{c.signal}"


def case_len(c):
    """F frames and a tail of H - 1 samples that no frame covers."""
    return N + (c.F - 1) * c.H + (c.H - 1)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def make_input(c):
    """x [C, L] float32, read-only: noise, or the two tones 120 dB apart, of welchutil.make_signals."""
    return _freeze(wu.make_signals(case_len(c), c.C, c.signal, seed=101 + CASES.index(c))[0])


@functools.lru_cache(maxsize=None)
def forward_reference(c):
    """stft64 of the case's input: complex128 [C, F, K], read-only."""
    return _freeze(sm.stft64(make_input(c), c.H, c.window))


@functools.lru_cache(maxsize=None)
def make_spectrum(c):
    """Z [C, F, K] complex64, read-only: seeded complex noise, no consistent STFT,
    with imaginary parts in bins 0 and 4096 that the inverse must ignore."""
    rng = np.random.default_rng(1001 + CASES.index(c))
    z = np.empty((c.C, c.F, K), np.complex64)
    for ch in range(c.C):
        z[ch] = (rng.standard_normal((c.F, K), np.float32) + 1j * rng.standard_normal((c.F, K), np.float32)) * (1.0 + ch)
    assert np.all(z[..., 0].imag != 0) and np.all(z[..., K - 1].imag != 0)
    return _freeze(z)


Envelope = namedtuple("Envelope", "den A hi lo band")


@functools.lru_cache(maxsize=None)
def envelope(F, H, window, floor=FLOOR):
    """den, A and the three sample classes of an output of full length: hi (den >=
    2 floor: the bound holds), lo (den < floor / 2: exactly 0) and the band between."""
    den, A = sm.envelope(F, H, window)
    hi, lo = den >= 2 * floor, den < floor / 2
    band = ~hi & ~lo
    idx = np.flatnonzero(band)
    # what the module's text says of the band: nothing with Hamming, the ends with Hann
    edges = np.concatenate([np.arange(F) * H, np.arange(F) * H + N - 1])
    near = np.min(np.abs(idx[:, None] - edges[None, :]), axis=1) if idx.size else idx
    assert idx.size == 0 or (window == "hann" and idx.size <= 6 * F and np.all(near < 16)), (F, H, window, idx)
    assert window != "hamming" or not lo.any()
    return Envelope(*_freeze(den, A, hi, lo, band))


Inverse = namedtuple("Inverse", "q vmax")


def quotient64(Z, H, window):
    """(num / den wherever den > 0, in float64, [C, Lfull]; max_f max |v_f| per row), a row at a time."""
    q, vmax = [], []
    for ch in range(Z.shape[0]):
        q.append(sm.istft64(Z[ch:ch + 1], H, window, floor=0.0)[0])
        vmax.append(np.max(np.abs(sm.frames64(Z[ch:ch + 1]))))
    return np.stack(q), np.array(vmax)


@functools.lru_cache(maxsize=None)
def inverse_reference(c):
    return Inverse(*_freeze(*quotient64(make_spectrum(c), c.H, c.window)))


def inverse_ratio(y, q, env, scale):
    """The rule of dsp_istft on y [C, n] against the float64 quotient q: samples of
    `lo` exactly 0; band samples 0 or within the bound; returns the worst
    |y - q| / A / scale[row] over `hi` and the band samples that are not 0."""
    y = np.asarray(y)
    n = y.shape[1]
    hi, lo, band, A = env.hi[:n], env.lo[:n], env.band[:n], env.A[:n]
    assert np.all(y[:, lo] == 0), "a sample below floor / 2 is not 0"
    e = np.abs(y.astype(np.float64) - q[:, :n])
    e[:, ~hi] = np.where(band[~hi] & (y[:, ~hi] != 0), e[:, ~hi], 0.0)
    m = hi | band
    return float(np.max(np.max(e[:, m] / A[m], axis=1) / scale))

