"""Models of the large real FFT, dsp_deconvolve and dsp_sweep (dspbench.h),
shared by the host, GPU and CLI tests and by tools/deconv_model.py.

float64: np.fft.rfft / irfft on float64 of the same float32 inputs, the
regularised division and the sweep's formula as the header writes them.

float32 (MODEL32): the device's pass arithmetic in complex64 -- the same
factorisation (plan), the same Stockham passes, the same two-level twiddle table
(float64 rounded once), the real split and the inverse split -- with the
radix-R transforms as radix-2 butterflies in complex64.  It is the yardstick
behind FFT_TOL and DEC_TOL: how far plain float32 arithmetic of this shape lands
from float64.

FFT_TOL and DEC_TOL are 4 x the worst MODEL32 error over the GPU tests' own
inputs (`tools/deconv_model.py tol` prints the figures below):

  e_fft = max_k |X32[k] - X64[k]| / max_k |X64[k]|   over fft_cases(n), n = 2^10..2^17, noise at 2^24,
          and the inverse of the float64 spectra relative to the row's peak
          worst 6.092e-07 (impulse at n/2 - 1, n = 2^17)  FFT_TOL = 2.44e-06
  e_dec = max_i |h32[i] - h64[i]| / max |h64|        over DEC_CASES (the peak of the whole response)
          worst 1.095e-04 (sweep, eps = 1e-12)           DEC_TOL = 4.38e-04
  recovery: the float64 model against the known band-limited h (sweep 50 Hz..20 kHz of
  0.5 s at 48 kHz with 10 ms fades, eps = 1e-6, h a band-pass biquad at 2 kHz, Q = 2):
          max |h64 - h| / max |h| = 1.241e-02 (the method: regularisation and the
          sweep's band edges); RECOVERY_TOL = 1.25 x = 1.55e-02

The MI355X's worst cases over the same inputs: e_fft 2.57e-07 (noise, n = 2^24),
e_dec 1.376e-04 (sweep, eps = 1e-12).
"""
import functools

import numpy as np

c64 = np.complex64
f32 = np.float32

FFT_TOL = 2.44e-06
DEC_TOL = 4.38e-04
RECOVERY_TOL = 1.55e-02

MIN_N, MAX_N = 1 << 10, 1 << 24
TW_SHIFT = 12  # W_n^K = hi[K >> 12] lo[K & 4095]


# ---------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------
def rfft_plan(n):
    """The radices of the M = n / 2 point transform, largest first: passes of
    64, with one or two of 32 and a last one of 8 where log2 M is no multiple of 6."""
    assert MIN_N <= n <= MAX_N and n & (n - 1) == 0
    m = n.bit_length() - 2  # log2 M
    p = -(-m // 6)
    d = 6 * p - m
    bits = [6] * p
    if d >= 3:
        bits[-1] = 3
        d -= 3
    for i in range(d):
        bits[p - 1 - (1 if bits[-1] == 3 else 0) - i] = 5
    bits.sort(reverse=True)
    assert sum(bits) == m
    return [1 << b for b in bits]


def deconv_n(Ly, Ls):
    n = 1024
    while n < max(Ly, Ls):
        n *= 2
    return n


def rfft_scratch_bytes(n):
    """Two buffers of M complex per channel."""
    return 2 * 8 * (n // 2)


def deconv_scratch_bytes(n, C):
    """A channel group's two work buffers and spectra, the excitation's spectrum, the word of the maximum."""
    g = min(C, 16)
    return g * rfft_scratch_bytes(n) + (g + 1) * 8 * (n // 2 + 1) + 16


# ---------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------
def rfft64(x, n):
    return np.fft.rfft(np.asarray(x, np.float64), n)


def deconv64(rec, ref, eps=1e-6, pre=0, ir_len=None):
    """ir [C, ir_len] in float64 from float32 rows, lambda as the header rounds it."""
    rec = np.atleast_2d(np.asarray(rec, f32))
    ref = np.asarray(ref, f32)
    n = deconv_n(rec.shape[1], ref.size)
    ir_len = n if ir_len is None else ir_len
    S = rfft64(ref, n)
    p = np.abs(S) ** 2
    lam = float(f32(eps)) * p.max()
    out = np.empty((rec.shape[0], ir_len))
    for c in range(rec.shape[0]):
        h = np.fft.irfft(rfft64(rec[c], n) * np.conj(S) / (p + lam), n)
        out[c] = h[(np.arange(ir_len) - pre) % n]
    return out


def sweep_len(sr, seconds):
    return int(np.floor(seconds * sr + 0.5))


def sweep64(sr, f1, f2, seconds, amplitude=1.0, fade=0):
    """The exponential sine sweep of dspbench.h in float64."""
    L = sweep_len(sr, seconds)
    R = np.log(f2 / f1)
    i = np.arange(L, dtype=np.float64)
    x = amplitude * np.sin(2.0 * np.pi * f1 * seconds / R * np.expm1(i / sr * R / seconds))
    if fade:
        w = 0.5 - 0.5 * np.cos(np.pi * (np.arange(fade) + 0.5) / fade)
        x[:fade] *= w
        x[L - fade:] *= w[::-1]
    return x


def harmonic_offset(sr, f1, f2, seconds, order):
    return seconds * np.log(order) / np.log(f2 / f1) * sr


# ---------------------------------------------------------------------------
# float32 (MODEL32)
# ---------------------------------------------------------------------------
@functools.lru_cache(4)
def twiddles(n):
    """(lo, hi) complex64: lo[k] = W_n^k, k < min(n, 4096); hi[h] = W_n^(4096 h)."""
    lo = np.exp(-2j * np.pi * np.arange(min(n, 1 << TW_SHIFT)) / n).astype(c64)
    hi = np.exp(-2j * np.pi * (np.arange(max(1, n >> TW_SHIFT)) << TW_SHIFT) / n).astype(c64)
    return lo, hi


def tw32(n, K):
    lo, hi = twiddles(n)
    return (hi[K >> TW_SHIFT] * lo[K & ((1 << TW_SHIFT) - 1)]).astype(c64)


def _dft32(v):
    """DFT along axis 0 (a power of two) as radix-2 butterflies in complex64."""
    R = v.shape[0]
    if R == 1:
        return v
    e, o = _dft32(v[0::2]), _dft32(v[1::2])
    w = np.exp(-2j * np.pi * np.arange(R // 2) / R).astype(c64).reshape((-1,) + (1,) * (v.ndim - 1))
    t = (w * o).astype(c64)
    return np.concatenate([e + t, e - t]).astype(c64)


def cfft32(z, n):
    """The M = n / 2 point complex transform of z (complex64) as the device's passes."""
    M = n // 2
    z = np.asarray(z, c64)
    Ns = 1
    for R in rfft_plan(n):
        Mr = M // R
        v = z.reshape(R, Mr)
        j = np.arange(Mr)
        if Ns > 1:
            K = 2 * ((j % Ns)[None, :] * np.arange(R)[:, None]) * (M // (Ns * R))
            v = (v * tw32(n, K)).astype(c64)
        V = _dft32(v)
        y = np.empty(M, c64)
        base = (j // Ns) * Ns * R + (j % Ns)
        y[base[None, :] + (np.arange(R) * Ns)[:, None]] = V
        z = y
        Ns *= R
    return z


def rfft32(x, n):
    """X[0..n/2] complex64 of a float32 row of L <= n samples."""
    M = n // 2
    xp = np.zeros(n, f32)
    xp[:len(x)] = np.asarray(x, f32)
    Z = cfft32(xp[0::2] + 1j * xp[1::2].astype(c64), n)
    k = np.arange(M + 1)
    a, b = Z[k % M], np.conj(Z[(M - k) % M])
    e = (f32(0.5) * (a + b)).astype(c64)
    o = (c64(-0.5j) * (a - b)).astype(c64)
    X = (e + tw32(n, k) * o).astype(c64)
    X[0] = c64(Z[0].real + Z[0].imag)
    X[M] = c64(Z[0].real - Z[0].imag)
    return X


def irfft32(X, n):
    """x[0..n) float32 of a complex64 spectrum of n / 2 + 1 bins."""
    M = n // 2
    X = np.asarray(X, c64).copy()
    X[0] = X[0].real
    X[M] = X[M].real
    k = np.arange(M)
    a, b = X[k], np.conj(X[M - k])
    Z = ((a + b) + c64(1j) * (np.conj(tw32(n, k)) * (a - b)).astype(c64)).astype(c64)
    w = cfft32(np.conj(Z), n)
    out = np.empty(n, f32)
    s = f32(1.0 / n)
    out[0::2] = w.real * s
    out[1::2] = -w.imag * s
    return out


def deconv32(rec, ref, eps=1e-6, pre=0, ir_len=None):
    rec = np.atleast_2d(np.asarray(rec, f32))
    n = deconv_n(rec.shape[1], len(ref))
    ir_len = n if ir_len is None else ir_len
    S = rfft32(ref, n)
    p = (S.real * S.real + S.imag * S.imag).astype(f32)
    lam = f32(f32(eps) * p.max())
    out = np.empty((rec.shape[0], ir_len), f32)
    for c in range(rec.shape[0]):
        Y = rfft32(rec[c], n)
        H = ((Y * np.conj(S)).astype(c64) / (p + lam).astype(f32)).astype(c64)
        h = irfft32(H, n)
        out[c] = h[(np.arange(ir_len) - pre) % n]
    return out


# ---------------------------------------------------------------------------
# the GPU tests' inputs
# ---------------------------------------------------------------------------
FFT_NS = tuple(1 << b for b in range(10, 18))
BIG_N = 1 << 24


def noise(seed, C, L):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (C, L)).astype(f32)


def decay(L, tau=300.0):
    return (np.exp(-np.arange(L) / tau) * np.cos(0.3 * np.arange(L))).astype(f32)


def impulse_positions(n):
    r = rfft_plan(n)[-1]
    return sorted({0, 1, 2, r - 1, r, r + 1, n // 2 - 1, n // 2, n - 1})


def cosine_bins(n):
    r = rfft_plan(n)[0]
    return sorted({0, 1, r - 1, r, r + 1, n // 4, n // 2})


def cosine(n, k):
    return np.cos(2.0 * np.pi * k * np.arange(n) / n).astype(f32)


def fft_cases(n):
    """(name, x float32 [L]) for the spectrum tests at n."""
    for j in impulse_positions(n):
        x = np.zeros(j + 1, f32)
        x[j] = 1.0
        yield f"impulse{j}", x
    for k in cosine_bins(n):
        yield f"cos{k}", cosine(n, k)
    yield "noise", noise(n, 1, n)[0]
    yield "decay", decay(n - 3)


def bandpass_ir(sr=48000, f0=2000.0, q=2.0, L=2048):
    """A band-pass biquad's impulse response (RBJ, constant 0 dB peak gain): band-limited inside a 50 Hz..20 kHz sweep."""
    w0 = 2.0 * np.pi * f0 / sr
    al = np.sin(w0) / (2.0 * q)
    b = np.array([al, 0.0, -al]) / (1.0 + al)
    a = np.array([1.0, -2.0 * np.cos(w0) / (1.0 + al), (1.0 - al) / (1.0 + al)])
    h = np.zeros(L)
    x = np.zeros(L)
    x[0] = 1.0
    for i in range(L):
        h[i] = b[0] * x[i] + (b[1] * x[i - 1] - a[1] * h[i - 1] if i >= 1 else 0.0) \
            + (b[2] * x[i - 2] - a[2] * h[i - 2] if i >= 2 else 0.0)
    return h.astype(f32)


SWEEP = dict(sr=48000, f1=50.0, f2=20000.0, seconds=0.5, amplitude=0.5, fade=480)  # `dspbench_render --sweep 50:20000:0.5`


def sweep32(**kw):
    return sweep64(**dict(SWEEP, **kw)).astype(f32)


def convolve(x, h, L):
    """x * h in float64, the first L samples as float32."""
    n = 1
    while n < len(x) + len(h):
        n *= 2
    y = np.fft.irfft(np.fft.rfft(np.asarray(x, np.float64), n) * np.fft.rfft(np.asarray(h, np.float64), n), n)
    return y[:L].astype(f32)


# name: excitation, Ly, Ls, eps, pre, ir_len (None: n)
DEC_CASES = [
    dict(name="sweep-eps6", exc="sweep", Ly=24000 + 2048, Ls=24000, eps=1e-6, pre=0, ir_len=None),
    dict(name="sweep-eps2-pre1", exc="sweep", Ly=24000 + 2048, Ls=24000, eps=1e-2, pre=1, ir_len=4096),
    dict(name="sweep-eps12-preall", exc="sweep", Ly=24000 + 2048, Ls=24000, eps=1e-12, pre=3000, ir_len=3000),
    dict(name="noise-eps12", exc="noise", Ly=4096, Ls=4096, eps=1e-12, pre=0, ir_len=None),
    dict(name="noise-eps6-len1", exc="noise", Ly=4096, Ls=4096, eps=1e-6, pre=0, ir_len=1),
    dict(name="noise-eps6-len1-pre1", exc="noise", Ly=4096, Ls=4096, eps=1e-6, pre=1, ir_len=1),
    dict(name="noise-past-pow2", exc="noise", Ly=4097, Ls=3000, eps=1e-6, pre=16, ir_len=None),
    dict(name="noise-ref-longer", exc="noise", Ly=1500, Ls=2049, eps=1e-2, pre=0, ir_len=2000),
]


def dec_case_input(k):
    """(rec [2, Ly], ref [Ls]) float32: the excitation through the known h (and through 0.5 h, delayed, on row 1)."""
    ref = sweep32() if k["exc"] == "sweep" else noise(k["Ls"], 1, k["Ls"])[0]
    assert ref.size == k["Ls"]
    h = bandpass_ir(L=1024)
    h2 = np.concatenate([np.zeros(5, f32), f32(0.5) * h])
    rec = np.stack([convolve(ref, h, k["Ly"]), convolve(ref, h2, k["Ly"])])
    return rec, ref
