"""The edge-value tables (edgevalues.py) and the oracle on them, on the CPU.

  * every tie is exactly (2k + 1) / 2^bits as a float32 (fractions.Fraction),
    and its expected code is round-half-to-even of k + 1/2, then the clip;
  * the oracle's float_to_pcm equals the integer expectation on every tie, on
    both float32 neighbours of every tie and on the clip edges; NaN encodes
    to 0 at every width (wav.h);
  * SPECIALS holds what its docstring says, per gain;
  * the oracle's render keeps denormals (oracle.c is built without fast-math:
    a flush-to-zero build would make the bit-exact GPU comparison blind to a
    flushing kernel).
"""
from fractions import Fraction

import numpy as np
import pytest

import edgevalues as ev

F32 = np.float32
TIES = {16: ev.ties16, 24: ev.ties24, 32: ev.ties32}


def _codes(oracle, x, nbits):
    """the oracle's codes of x as signed integers"""
    raw = np.asarray(oracle.float_to_pcm(np.ascontiguousarray(x, F32), nbits)).view(np.uint8).reshape(-1, nbits // 8)
    v = sum(raw[:, b].astype(np.int64) << (8 * b) for b in range(nbits // 8))
    return np.where(v >= 1 << (nbits - 1), v - (1 << nbits), v)


@pytest.mark.parametrize("nbits", [16, 24, 32])
def test_ties_are_exact_halves(nbits):
    x, code = TIES[nbits]()
    assert x.dtype == F32 and code.shape == x.shape
    scale = 1 << (nbits - 1)
    lo, hi = -scale, scale - 1
    step = max(1, x.size // 20_000)          # Fraction is slow: every tie at 16 bits, a stride elsewhere,
    idx = np.unique(np.concatenate([np.arange(0, x.size, step), np.arange(min(64, x.size)),
                                    np.arange(x.size - min(64, x.size), x.size)]))
    for i in idx:
        v = Fraction(float(x[i])) * scale        # exact: a float is a dyadic rational
        assert v.denominator == 2, (nbits, i, x[i])
        k = (v.numerator - 1) // 2               # v = k + 1/2
        want = k if k % 2 == 0 else k + 1
        assert code[i] == max(lo, min(hi, want)), (nbits, i, x[i])
    # and all of them, vectorised: x 2^(bits-1) is exact in float64
    v = x.astype(np.float64) * scale
    assert np.all(v - np.floor(v) == 0.5)
    assert np.array_equal(code, np.clip(np.rint(v).astype(np.int64), lo, hi))   # numpy's rint is half to even


def test_tie_tables_cover_what_they_claim():
    x16, c16 = ev.ties16()
    assert x16.size == 65_537 and c16.min() == -32768 and c16.max() == 32767
    assert x16[0] * 32768 == -32768.5 and x16[-1] * 32768 == 32767.5    # one tie past each clip edge
    x24, c24 = ev.ties24()
    v = x24.astype(np.float64) * (1 << 23)
    assert v.min() == -(1 << 23) + 0.5 and v.max() == (1 << 23) - 0.5
    assert c24.min() == -(1 << 23) and c24.max() == (1 << 23) - 1
    assert np.count_nonzero(np.abs(v) <= (1 << 16) + 0.5) >= 2 * (1 << 16) + 1
    x32, _ = ev.ties32()
    assert x32.size == 2 * (1 << 16) - 1


@pytest.mark.parametrize("nbits", [16, 24, 32])
def test_oracle_encode_on_ties_neighbours_and_edges(oracle, nbits):
    x, code = TIES[nbits]()
    assert np.array_equal(_codes(oracle, x, nbits), code)
    nb = ev.neighbours(x)
    if nbits == 16:
        want = ev.expected_codes(nb, nbits)                  # exact arithmetic on all 131,074
    else:
        # a neighbour is off the tie by less than 1/2: it rounds to the nearer
        # of k and k + 1; exact arithmetic on a stride confirms the shortcut
        k = np.floor(x.astype(np.float64) * (1 << (nbits - 1))).astype(np.int64)
        want = np.clip(np.concatenate([k, k + 1]), -(1 << (nbits - 1)), (1 << (nbits - 1)) - 1)
        s = slice(0, None, max(1, nb.size // 5_000))
        assert np.array_equal(want[s], ev.expected_codes(nb[s], nbits))
    assert np.array_equal(_codes(oracle, nb, nbits), want)
    ex, ecode = ev.clip_edges(nbits)
    assert np.array_equal(_codes(oracle, ex, nbits), ecode)
    top, bot = (1 << (nbits - 1)) - 1, -(1 << (nbits - 1))
    # (1 - 2^-24 still rounds to full scale at 16 and 24 bits; at 32 bits it is 2^31 - 128 exactly)
    assert list(ecode[:4]) == [top, bot, top if nbits < 32 else top - 127, bot if nbits < 32 else bot + 128]
    assert list(ecode[4:10]) == [1, -1, top, bot, top, bot] and not np.any(ecode[10:])


@pytest.mark.parametrize("nbits", [16, 24, 32])
def test_oracle_encodes_nan_to_zero(oracle, nbits):
    nans = np.array([0x7FC00000, 0xFFC00000, ev.QNAN_BITS, 0x7F800001, 0xFFFFFFFF], np.uint32).view(F32)
    assert not np.any(_codes(oracle, nans, nbits))
    # float encode stays a byte copy
    assert np.array_equal(np.asarray(oracle.float_to_pcm(nans, 32, True)).view(np.uint32).ravel(), nans.view(np.uint32))


def _b(v):
    return int(np.array([v], F32).view(np.uint32)[0])


def test_specials_hold_what_they_claim():
    s = ev.SPECIALS
    b = set(ev.bits(s).tolist())
    for v in (0.0, ev.DEN_MIN, ev.DEN_MAX, ev.FLT_MIN, ev.FLT_MAX, np.inf, 1.0, ev.ONE_BELOW):
        assert _b(v) in b and _b(-v) in b, v
    assert ev.QNAN_BITS in b and np.isnan(ev.QNAN) and ev.QNAN_BITS & 0x3FFFFF
    assert float(ev.DEN_MAX) == 2.0 ** -126 - 2.0 ** -149 and float(ev.ONE_BELOW) == 1 - 2.0 ** -24
    with np.errstate(over="ignore", under="ignore"):
        for g in ev.GAINS:
            cases = ev.gain_cases(g)
            assert "denormal" in cases and ("zero" in cases) == (g < 0.5) and ("inf" in cases) == (g > 1)
            for kind, vals in cases.items():
                for v in vals:
                    assert _b(v) in b and _b(-v) in b
                    p = F32(v) * F32(g)
                    ok = {"denormal": 0 < abs(p) < ev.FLT_MIN, "zero": p == 0 and v != 0, "inf": np.isinf(p)}[kind]
                    assert ok, (g, kind, v, p)


def test_same_bits_nan():
    a = np.array([0.0, 1.0, np.nan, ev.DEN_MIN], F32)
    assert ev.same_bits_nan(a, a.copy())
    assert ev.same_bits_nan(a, np.array([0.0, 1.0, -ev.QNAN, ev.DEN_MIN], F32))      # any NaN is any NaN
    assert not ev.same_bits_nan(a, np.array([-0.0, 1.0, np.nan, ev.DEN_MIN], F32))   # the sign of zero counts
    assert not ev.same_bits_nan(a, np.array([0.0, 1.0, np.nan, 0.0], F32))
    assert not ev.same_bits_nan(a, np.array([0.0, 1.0, 1.0, ev.DEN_MIN], F32))
    assert not ev.same_bits(a, np.array([0.0, 1.0, ev.QNAN, ev.DEN_MIN], F32))       # plain: payloads count


@pytest.mark.parametrize("pname,gain", [("gain_test", 0.2), ("static_gain_plugin", 0.1), ("no_op", None)])
def test_oracle_render_keeps_denormals(oracle, pname, gain):
    """oracle.c's render on seeded rows against float32 numpy: denormal inputs
    and denormal products survive, signed zeros keep their sign, NaN stays NaN."""
    L_, B = 1_031, 100
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (2, L_)).astype(F32)
    pos = ev.positions(L_, B, rng)
    x = ev.seeded(x, ev.SPECIALS, pos)
    got = oracle.render_offline([x[0], x[1]], 2, B, 48000.0, oracle.restated_plugin(pname))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        want = x if gain is None else x * F32(gain)
    assert ev.same_bits_nan(got[:, :L_], want), ev.first_diff(got[:, :L_], want)
    assert not np.any(got[:, L_:])
    den = (np.abs(want) > 0) & (np.abs(want) < ev.FLT_MIN)
    assert np.count_nonzero(den) >= 8          # the case is not vacuous
    assert np.all(got[:, :L_][den] != 0)
