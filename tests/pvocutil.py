"""Shapes, inputs, references and the tolerance of the dsp_pvoc and
dsp_time_stretch tests (test_pvoc_host.py, test_gpu_pvoc.py).  The float64
references come from tools/pvoc_model.py and are computed once per case.

PVOC_TOL: per bin |Z' - Z'64| <= PVOC_TOL sqrt(t + 1) |Z'64| + ulp32(the frame's
largest |Z'64|), every bin of every frame (pvoc_model.ratio).  It is 4 x the
larger of two worst ratios measured over exactly CASES, the way STFT_TOL and
WELCH_TOL were set; the factor 4 covers inputs not in the list.
  the float32 CPU model (pvoc_model.pvoc32 against pvoc64):  MODEL_RATIO
  the GPU (dsp_pvoc against pvoc64, MI355X):                 GPU_RATIO
The sqrt shape is the random walk of the rounded arguments; over these short
cases (t <= 128) the first frames set both ratios: one argument's and one
sin / cos's rounding, about 2e-7.

STRETCH_TOL: dsp_time_stretch against stft64, pvoc64, istft64 on sums of
bin-centred tones of comparable level, in the inverse's shape: per row
|y - y64| <= STRETCH_TOL A[i] max |y64| over the samples with den >= 2 floor
(cstftutil.inverse_ratio, the Hann floor band named there taken either way).
4 x the larger of STRETCH_MODEL_RATIO (stft32, pvoc32, istft32) and
STRETCH_GPU_RATIO over STRETCH_CASES.
"""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import pvoc_model as pm  # noqa: E402

N, K = pm.N, pm.K
MAXCH = 16
CHUNK = 64  # dsp_pvoc_plan's chunk; the tests assert it

MODEL_RATIO = 1.54e-7
GPU_RATIO = 1.19e-7
PVOC_TOL = 4.0 * max(MODEL_RATIO, GPU_RATIO)

STRETCH_MODEL_RATIO = 2.23e-7
STRETCH_GPU_RATIO = 2.90e-7
STRETCH_TOL = 4.0 * max(STRETCH_MODEL_RATIO, STRETCH_GPU_RATIO)

Case = namedtuple("Case", "F rate C")

# two output frames, the second against the zero pad; the smallest recurrence;
# a rate above 1; frames skipped; pairs repeated; chunk + 1 output frames (the
# seam); two chunks + 1 on 17 channels (two channel groups, two carries)
CASES = [Case(1, 0.5, 1), Case(2, 1.0, 1), Case(5, 1.25, 2), Case(7, 3.0, 1), Case(6, 0.3, 3),
         Case(52, 0.8, 2), Case(162, 1.2599, 17)]
assert pm.frames_out(52, 0.8) == CHUNK + 1 and pm.frames_out(162, 1.2599) == 2 * CHUNK + 1
assert pm.frames_out(1, 0.5) == 2
SEAM = CASES[5]


def case_id(c):
    return f"F{c.F}-r{c.rate}-C{c.C}"


def _freeze(a):
    a.setflags(write=False)
    return a


def random_spectrum(F, C, seed, zeros=True):
    """Z [C, F, K] complex64: seeded complex noise, every seventh bin 120 dB down,
    and imaginary parts in bins 0 and 4096 (all bins are treated alike); with
    `zeros`, bin 11 zero in every frame and bins 5 (mod 13) zero in frame 1 (mod 3)."""
    rng = np.random.default_rng(seed)
    z = np.empty((C, F, K), np.complex64)
    for ch in range(C):
        z[ch] = (rng.standard_normal((F, K), np.float32) + 1j * rng.standard_normal((F, K), np.float32)) * (1.0 + ch % 3)
    z[:, :, ::7] *= np.float32(1e-6)
    if zeros:
        z[:, :, 11] = 0
        z[:, 1::3, 5::13] = 0
    return z


@functools.lru_cache(maxsize=None)
def make_spectrum(c):
    return _freeze(random_spectrum(c.F, c.C, 2001 + CASES.index(c)))


@functools.lru_cache(maxsize=None)
def reference(c):
    """pvoc64 of the case's spectrum: complex128 [C, F', K], read-only."""
    return _freeze(pm.pvoc64(make_spectrum(c), c.rate))


# ---------------------------------------------------------------------------
# dsp_time_stretch: sums of bin-centred tones of comparable level
# ---------------------------------------------------------------------------
StretchCase = namedtuple("StretchCase", "F H rate C")
STRETCH_CASES = [StretchCase(9, 2048, 0.8, 2), StretchCase(9, 2048, 1.25, 2), StretchCase(17, 512, 0.8, 1)]
TONE_BINS = (96, 1000, 2511, 3900)


def stretch_id(c):
    return f"F{c.F}-H{c.H}-r{c.rate}-C{c.C}"


def stretch_len(c):
    return N + (c.F - 1) * c.H


def tones(L, bins, amps, phases):
    n = np.arange(L, dtype=np.float64)
    x = sum(a * np.cos(2 * np.pi * k * n / N + p) for k, a, p in zip(bins, amps, phases))
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def stretch_input(c):
    """x [C, L] float32: four bin-centred tones per channel, amplitudes within 6 dB of each other."""
    L = stretch_len(c)
    rows = [tones(L, TONE_BINS, (0.2, 0.15, 0.25, 0.1), (0.1 + ch, 1.0 - ch, 2.0, -0.7 * (ch + 1))) for ch in range(c.C)]
    return _freeze(np.stack(rows))


@functools.lru_cache(maxsize=None)
def stretch_reference(c):
    """The float64 chain at full length: float64 [C, Lout_full]."""
    return _freeze(pm.stretch64(stretch_input(c), c.rate, c.H, "hann", None, 0.0))


def stretch_ratio(y, c):
    """dsp_time_stretch's output y [C, n] against the float64 chain, in dsp_istft's shape."""
    import cstftutil as cu
    q = stretch_reference(c)
    env = cu.envelope(pm.frames_out(c.F, c.rate), c.H, "hann")
    return cu.inverse_ratio(y, q, env, np.max(np.abs(q), axis=1))
