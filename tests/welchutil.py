"""Shapes, signals, references and the tolerance of the dsp_welch tests
(test_welch_host.py, test_gpu_welch.py).  The float64 references come from
tools/welch_model.py and are computed once per case.

WELCH_TOL: per row max_k |S - S64| <= WELCH_TOL max_k S64 (for sxy the scale is
sqrt(max sxx max srr)).  It is 4 x the larger of two worst ratios measured over
exactly CASES, the way CONV_TOL was set; the factor 4 covers inputs not in the
list.
  float32 CPU model (tools/welch_model.py sums32 against sums64): MODEL_RATIO
  the GPU (dsp_welch against sums64, MI355X):                      GPU_RATIO
"""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import welch_model as wm  # noqa: E402

N, K, RUN = wm.N, wm.K, wm.RUN
MAXCH = 16  # kMaxChannels

MODEL_RATIO = 2.82e-7
GPU_RATIO = 3.68e-7
WELCH_TOL = 4.0 * max(MODEL_RATIO, GPU_RATIO)


def chunk_frames(C, has_ref):
    """The plan's chunk for a call long enough to need one: the largest multiple
    of RUN whose spectra (33792 bytes a frame and row) fit 64 MiB."""
    rows = min(C, MAXCH) + (1 if has_ref else 0)
    return max((64 << 20) // (rows * 33792) // RUN, 1) * RUN


def scratch_bytes(F, C, has_ref):
    cn = min(C, MAXCH)
    chunk = min(chunk_frames(C, has_ref), (F + RUN - 1) // RUN * RUN)
    runs = chunk // RUN
    return (cn + (1 if has_ref else 0)) * chunk * 33792 + cn * runs * 2112 * 8 + \
        ((cn * runs * 2112 * 16 + runs * 2112 * 8) if has_ref else 0)


Case = namedtuple("Case", "F H C window ref signal")

# F across every boundary of the order (1, 2, run - 1, run, run + 1, 2 run + 1,
# one chunk + 1 -- the chunk depends on the rows), every hop, every channel
# count, both windows, with and without the reference, both signals.  The large
# F ride on H = 1 so that L stays small.
CASES = [
    Case(1, 4096, 1, "hann", True, "noise"),
    Case(2, 4096, 2, "hamming", False, "noise"),
    Case(RUN - 1, 8192, 1, "hann", True, "noise"),
    Case(RUN, 4095, 2, "hann", True, "noise"),
    Case(RUN + 1, 2730, 3, "hamming", True, "noise"),
    Case(2 * RUN + 1, 4096, 1, "hann", False, "noise"),
    Case(2 * RUN + 1, 1, MAXCH + 1, "hann", True, "noise"),
    Case(chunk_frames(1, False) + 1, 1, 1, "hann", False, "noise"),
    Case(chunk_frames(2, True) + 1, 1, 2, "hamming", True, "noise"),
    Case(chunk_frames(MAXCH + 1, True) + 1, 1, MAXCH + 1, "hann", True, "noise"),
    Case(RUN + 1, 4096, 1, "hann", False, "tones"),
    Case(RUN, 4095, 2, "hamming", True, "tones"),
]

FIR3 = np.array([1.0, 0.5, -0.25])


def case_id(c):
    return f"F{c.F}-H{c.H}-C{c.C}-{c.window}-{'ref' if c.ref else 'noref'}-{c.signal}"


def case_len(c):
    """F frames and a tail of H - 1 samples that no frame covers."""
    return N + (c.F - 1) * c.H + (c.H - 1)


def make_signals(L, C, signal="noise", seed=1):
    """ref [L]: seeded white noise (or two tones 120 dB apart).  x[c]: ref through
    a known 3-tap FIR, scaled per channel, plus independent noise 20 dB below the
    reference, so the coherence lies strictly between 0 and 1."""
    rng = np.random.default_rng(seed)
    if signal == "noise":
        ref = 0.25 * rng.standard_normal(L)
    else:
        n = np.arange(L)
        ref = 0.5 * np.sin(2 * np.pi * 0.0501 * n) + 0.5e-6 * np.sin(2 * np.pi * 0.2003 * n + 0.3)
    x = np.empty((C, L))
    for c in range(C):
        y = np.convolve(ref, FIR3)[:L] * (1.0 - 0.03 * c)
        x[c] = y + 0.1 * np.std(ref) * rng.standard_normal(L)
    return x.astype(np.float32), ref.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(c):
    x, ref = make_signals(case_len(c), c.C, c.signal, seed=1 + CASES.index(c) if c in CASES else 99)
    x.setflags(write=False)
    ref.setflags(write=False)
    want = wm.sums64(x, ref if c.ref else None, c.H, c.window)
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return x, ref, want


def make_case(c):
    """(x [C, L], ref [L] or None) float32, read-only."""
    x, ref, _ = _case(c)
    return x, (ref if c.ref else None)


def reference(c):
    """sums64 of the case: (sxx, srr, sxy complex) read-only, shared by the tests."""
    return _case(c)[2]


def as_model(sxx, srr, sxy):
    """The library's rows (sxy interleaved) in welch_model's form (sxy complex)."""
    return np.asarray(sxx), srr, (None if sxy is None else np.ascontiguousarray(sxy).view(np.complex128))
