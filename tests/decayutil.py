"""Shapes, signals, references and the tolerance of the dsp_decay tests
(test_decay_host.py, test_gpu_decay.py, test_cli_decay.py).  The float64
references come from tools/decay_model.py and are computed once per case.

DECAY_TOL: per energy row max_j |e - e64| <= DECAY_TOL max_j e64, entry 0
included (moments: the same bound times L).  It is 4 x the larger of two worst
ratios measured over exactly CASES, the way WELCH_TOL and CONV_TOL were set; the
factor 4 covers inputs not in the list.
  float32 CPU model (tools/decay_model.py energies32 against energies64): MODEL_RATIO
  the GPU (dsp_decay against energies64, MI355X):                         GPU_RATIO
"""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import decay_model as dm  # noqa: E402

MAXCH = 16  # kMaxChannels: rows per launch group

MODEL_RATIO = 6.343e-7
GPU_RATIO = 8.636e-7
DECAY_TOL = 4.0 * max(MODEL_RATIO, GPU_RATIO)

OCT_HIGH = (1, 3, 3)        # one high octave (7.9 kHz): P = 69 at 48 kHz
OCTAVES = (1, -5, 4)        # the octave default, 10 bands
OCT7 = (1, -3, 3)           # 126 Hz .. 7.9 kHz: fits 44.1 kHz
THIRDS32 = (3, -18, 13)     # 32 third-octave bands, 15.8 Hz .. 20 kHz

# name, L, sr, bands, C, signal, lead (zeros before the first, loudest sample: the onset)
Case = namedtuple("Case", "name L sr bands C signal lead")


def _P(sr, bands):
    return dm.plan(1, sr, *bands)["P"]


def _cases():
    P48 = _P(48000, OCT_HIGH)
    c = [
        Case("smallest", 700, 48000, OCT_HIGH, 1, "noise", 5),                  # n = 1024
        Case("n-at-pow2", 2048 - P48, 48000, OCT_HIGH, 1, "noise", 9),          # L + P = 2^11
        Case("n-past-pow2", 2048 - P48 + 1, 48000, OCT_HIGH, 2, "noise", 9),    # L + P = 2^11 + 1: n = 4096
        Case("onset0", 1500, 48000, OCT_HIGH, 1, "noise", 0),
        Case("impulse-last", 1501, 48000, OCT_HIGH, 1, "impulse", 1500),        # one partial hop of one sample
        Case("hop-rem0", 100 + 30 * 48, 48000, OCT_HIGH, 1, "noise", 100),      # (L - onset) % hop = 0
        Case("hop-rem1", 100 + 30 * 48 + 1, 48000, OCT_HIGH, 1, "noise", 100),
        Case("hop-rem47", 100 + 30 * 48 + 47, 48000, OCT_HIGH, 1, "noise", 100),
        Case("hop21-rem20", 50 + 40 * 21 + 20, 44100, OCT_HIGH, 2, "noise", 50),
        Case("C2-b10", 5000, 48000, OCTAVES, 2, "noise", 333),                  # 20 rows: two groups, one across channels
        Case("C17-b32", 3000, 48000, THIRDS32, MAXCH + 1, "noise", 64),         # two channel groups, 34 row groups
        Case("sines-48k", 72000, 48000, OCT7, 1, "sines", 37),
        Case("sines-44k1", 66150, 44100, OCT7, 1, "sines", 37),
    ]
    return c


CASES = _cases()


def case_id(c):
    return c.name


def make_signal(c, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((c.C, c.L), np.float32)
    if c.signal == "impulse":
        x[:, c.lead] = 0.75
    elif c.signal == "sines":
        assert c.lead == 37
        x[:] = dm.decaying_sines(c.sr, c.L / c.sr, c.lead)
    else:
        n = c.L - c.lead
        t = np.arange(n) / c.sr
        for ch in range(c.C):
            v = 0.2 * rng.standard_normal(n) * np.exp(-6.9 * t / (0.02 + 0.01 * ch))
            v = np.clip(v, -0.7, 0.7)
            v[0] = 0.8 - 0.01 * ch  # the loudest sample comes first: onset = lead, exactly
            x[ch, c.lead:] = v
    return x


@functools.lru_cache(maxsize=None)
def _case(c):
    x = make_signal(c, 1 + CASES.index(c) if c in CASES else 99)
    x.setflags(write=False)
    want = dm.energies64(x, c.sr, *c.bands)
    for a in want:
        a.setflags(write=False)
    return x, want


def make_case(c):
    """x [C, L] float32, read-only."""
    return _case(c)[0]


def reference(c):
    """energies64 of the case: (peak, onset, energy, moment), read-only, shared by the tests."""
    return _case(c)[1]


def expected_onset(c):
    """The onset by construction: 38 for the sines (their sample 37 is sin 0), else the lead."""
    return c.lead + 1 if c.signal == "sines" else c.lead


def check_energies(got_e, got_m, want_e, want_m, L, tol=None):
    """The bound on every row; returns the worst energy ratio."""
    tol = DECAY_TOL if tol is None else tol
    scale = want_e.max(axis=-1)
    re = np.max(np.abs(got_e - want_e), axis=-1)
    assert np.all(re <= tol * scale), float(np.max(re / np.where(scale > 0, scale, 1)))
    if got_m is not None:
        rm = np.max(np.abs(got_m - want_m), axis=-1)
        assert np.all(rm <= tol * L * scale), float(np.max(rm / np.where(scale > 0, L * scale, 1)))
    return dm.ratios(got_e, want_e)
