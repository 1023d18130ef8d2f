"""Float edge values for the tests: the float32 values at which a kernel and
its reference can part ways without any random input ever showing it, and the
PCM encoder's rounding ties with their codes worked out in integer arithmetic.

SPECIALS   +-0, the smallest and the largest denormal, FLT_MIN, FLT_MAX, +-inf,
           a quiet NaN with a payload, +-1, +-(1 - 2^-24), and for every gain in
           GAINS the inputs whose product with it is a denormal, rounds to zero
           or overflows.  Not every gain has all three: a gain below 1 cannot
           take a finite float past FLT_MAX (the overflow inputs belong to the
           in-place dsp_gain by 2.0), and 0.7 x >= 2^-149 for every non-zero x
           (no product with 0.7 rounds to zero).  gain_cases() says which
           inputs do what, test_edge_values_cpu.py checks the table.
seeded     a copy of a row with specials written at chosen indices.
same_bits_nan   bit-for-bit equality where any NaN equals any NaN (arithmetic
           may change a NaN's payload and sign); the sign of zero counts.
ties16/24/32   (x float32, expected code): every x is exactly (2k + 1) / 2^bits,
           so x 2^(bits-1) = k + 1/2, and the code is round-half-to-even of
           that, then the clip to [-2^(bits-1), 2^(bits-1) - 1].
"""
from fractions import Fraction

import numpy as np

F32 = np.float32
DEN_MIN = F32(2.0 ** -149)
DEN_MAX = np.array([0x007FFFFF], np.uint32).view(F32)[0]
FLT_MIN = F32(2.0 ** -126)
FLT_MAX = np.finfo(F32).max
QNAN_BITS = 0x7FC12345
QNAN = np.array([QNAN_BITS], np.uint32).view(F32)[0]
ONE_BELOW = F32(1.0 - 2.0 ** -24)

# the gains of the render tests (gain_test, static_gain, test_render_unaligned_
# scalar_path, the elementwise services) and the in-place dsp_gain's 2.0
GAINS = (0.2, 0.1, 0.7, 0.37, 2.0)


def gain_cases(g):
    """{"denormal" | "zero" | "inf": positive float32 inputs whose float32
    product with float32(g) is a denormal / zero / infinite}"""
    if g < 1:
        out = {"denormal": [FLT_MIN, F32(1.25 * 2.0 ** -126), F32(2.0 ** -130)]}
        if g < 0.5:
            out["zero"] = [DEN_MIN, F32(2 * 2.0 ** -149)] if g < 0.25 else [DEN_MIN]
    else:
        out = {"denormal": [DEN_MIN, F32(2.0 ** -128)],
               "inf": [FLT_MAX, F32(2.0 ** 127), F32(1.5 * 2.0 ** 127)]}
    return out


def _specials():
    base = [0.0, DEN_MIN, DEN_MAX, FLT_MIN, FLT_MAX, np.inf, 1.0, ONE_BELOW]
    for g in GAINS:
        for vals in gain_cases(g).values():
            base += vals
    pos = np.array(base, F32)
    both = np.stack([pos, -pos], 1).ravel()            # +v, -v for each
    return np.concatenate([both, np.array([QNAN], F32)])


SPECIALS = _specials()
SPECIALS.setflags(write=False)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def seeded(x, specials, positions):
    """x with specials[i % len] written at positions[i]; positions may hold
    negative indices (from the end).  The input is left alone."""
    y = np.array(x, F32, copy=True)
    pos = np.asarray(positions, np.int64)
    y[..., pos] = np.resize(np.asarray(specials, F32), pos.size)
    return y


def positions(L, block, rng, extra=50):
    """The first 4 samples, the last L % 4 (at least 1), four on either side of
    the first block edge, and `extra` seeded indices: sorted, unique."""
    tail = max(L % 4, 1)
    p = list(range(4)) + list(range(L - tail, L))
    if block + 4 <= L:
        p += list(range(block - 4, block + 4))
    p += list(rng.integers(4, L - tail, extra))
    return np.unique(np.asarray(p, np.int64))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_bits_nan(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def first_diff(a, b):
    """for an assertion message: (flat index, a's bits, b's bits) of the first difference"""
    a, b = bits(a).ravel(), bits(b).ravel()
    i = int(np.argmax(a != b))
    return i, hex(int(a[i])), hex(int(b[i]))


# ---------------------------------------------------------------------------
# PCM encode: ties and clip edges
# ---------------------------------------------------------------------------
def half_even_clip(v: Fraction, nbits: int) -> int:
    """round-half-to-even of the exact value v, then the clip to nbits"""
    fl = v.numerator // v.denominator
    r = v - fl
    n = fl + 1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and fl % 2) else fl
    return max(-(1 << (nbits - 1)), min((1 << (nbits - 1)) - 1, n))


def expected_code(x, nbits: int) -> int:
    """The code of one float32 sample by the rule of wav.h, in exact arithmetic."""
    x = float(x)
    if x != x:
        return 0
    if x in (float("inf"), float("-inf")):
        return (1 << (nbits - 1)) - 1 if x > 0 else -(1 << (nbits - 1))
    return half_even_clip(Fraction(x) * (1 << (nbits - 1)), nbits)


def expected_codes(x, nbits: int) -> np.ndarray:
    return np.array([expected_code(v, nbits) for v in np.asarray(x, F32).ravel()], np.int64)


def _ties(k, nbits):
    """x = (2k + 1) / 2^nbits as float32 (exact while 2k + 1 < 2^24 in
    magnitude, which the CPU test checks) and the code of k + 1/2: the even one
    of k and k + 1, clipped."""
    k = np.asarray(k, np.int64)
    x = ((2 * k + 1).astype(np.float64) * 2.0 ** -nbits).astype(F32)
    code = np.where(k % 2 == 0, k, k + 1)
    return x, np.clip(code, -(1 << (nbits - 1)), (1 << (nbits - 1)) - 1)


def ties16():
    """all 65,537 ties k + 1/2, k in [-32769, 32767]: one past each clip edge"""
    return _ties(np.arange(-32769, 32768), 16)


def ties24(rng=None):
    """ties with |k| <= 2^16, the ties within 2^16 of +-2^23 (2k + 1 must stay
    below 2^24 to be a float32: -2^23 + 1/2 and 2^23 - 1/2 are the outermost
    ties, and the latter rounds to 2^23 and clips), and 2^16 seeded ones"""
    rng = np.random.default_rng(24) if rng is None else rng
    k = np.concatenate([np.arange(-(1 << 16), (1 << 16) + 1),
                        np.arange(-(1 << 23), -(1 << 23) + (1 << 16)),
                        np.arange((1 << 23) - (1 << 16), 1 << 23),
                        rng.integers(-(1 << 23), 1 << 23, 1 << 16)])
    return _ties(k, 24)


def ties32():
    """ties with |k| < 2^16 (beyond |k| = 2^23 a float32 holds no half)"""
    return _ties(np.arange(-(1 << 16) + 1, 1 << 16), 32)


def neighbours(x):
    """both float32 neighbours of every x"""
    x = np.asarray(x, F32)
    return np.concatenate([np.nextafter(x, F32(-np.inf)), np.nextafter(x, F32(np.inf))])


def clip_edges(nbits):
    """(x, code): +-1 and their inward neighbours, +-2^-(nbits-1) (one code),
    +-FLT_MAX, +-inf, +-0, denormals and NaN"""
    lsb = F32(2.0 ** -(nbits - 1))
    x = np.array([1.0, -1.0, np.nextafter(F32(1), F32(0)), np.nextafter(F32(-1), F32(0)), lsb, -lsb,
                  FLT_MAX, -FLT_MAX, np.inf, -np.inf, 0.0, -0.0, DEN_MIN, -DEN_MIN, DEN_MAX, -DEN_MAX, QNAN], F32)
    return x, expected_codes(x, nbits)


def codes_to_bytes(codes, nbits):
    """little-endian two's-complement payload bytes of integer codes"""
    c = np.asarray(codes, np.int64) & ((1 << nbits) - 1)
    return np.stack([(c >> (8 * b)) & 0xFF for b in range(nbits // 8)], 1).astype(np.uint8).ravel()
