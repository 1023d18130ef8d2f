"""Which values the rows hold: rounding ties and clip edges of the PCM encoder,
denormals, signed zeros, FLT_MAX, infinities and NaN through every bit-exact
family, power-of-two homogeneity of the linear kernels, quiet and loud STFT
frames against float64, and the second trip of the generic WAV kernels' loops.
Every other GPU test draws from uniform(-1, 1) or random PCM codes; the tables
and comparisons are edgevalues.py's (checked on the CPU by
test_edge_values_cpu.py).

  a. encode: the code of every tie, of both neighbours of the int16 ties and of
     the clip edges equals the integer expectation (half to even, then clip;
     NaN -> 0) and the oracle, in the tile kernels (C = 1, 2), the generic one
     (C = 3) and the partial last group.
  b. the bit-exact families on rows seeded with SPECIALS, against the oracle's
     restated plugins (oracle.c, built without fast-math) or float32 numpy.
     Arithmetic results compare with same_bits_nan (any NaN is any NaN, the
     sign of zero counts); copies compare in every bit, NaN payloads included.
  c. f(2^k x) = 2^k f(x) bit for bit (2^2k for energies), k = -20 and +20, for
     every linear kernel.  The claim is sound when nothing under- or overflows:
     each case first asserts that no non-zero value of the k = 0 result lies
     below 2^-60 (an exact zero scales to the same zero, sign included).
  d. STFT magnitudes of frames scaled by 2^-30 .. 2^-100 and 2^+40 against
     float64, per frame max|m - ref| <= PEAK_REL_TOL peak + 2^-61: the raw
     square root flushes a denormal argument (re^2 + im^2, or a quarter of it),
     so a magnitude below 2^-62 may be stored as zero (dspbench.h); and the
     biquad kind's impulse response decaying through the denormals to zero.
  e. 16-bit, 3 channels: a decode of more than 4096 x 256 groups of 4 frames
     and an encode of more than 4096 x 256 samples (wav.hip grid_for).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L
import edgevalues as ev
import loudnessutil as lu
import resampleutil as rsu
import rowsutil as ru
from convutil import conv_inputs
from test_gpu_biquad import check as biquad_check, random_cascade
from test_gpu_parity import PEAK_REL_TOL, PLUGINS, rnd
from test_gpu_rows import biquad_inputs, fir_inputs
from test_gpu_wav import _info as wav_info

pytestmark = pytest.mark.gpu

F32 = np.float32
SR = 48000.0
TIES = {16: ev.ties16, 24: ev.ties24, 32: ev.ties32}


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def sync_exec(torch):
    return L.dsp_exec(torch.cuda.current_device(), L.DSP_EXEC_SYNC, C.c_void_p(torch.cuda.current_stream().cuda_stream), 0)


# ---------------------------------------------------------------------------
# a. encode edges
# ---------------------------------------------------------------------------
@functools.lru_cache(None)
def encode_vector(nbits):
    """(x, code): 16 ties again in front (a case may drop up to 11 leading
    samples to end in a partial group), the ties, the clip edges, at 16 bits
    both neighbours of every tie, and 64 ties last: the last, partial group of
    4 frames holds ties."""
    tx, tc = TIES[nbits]()
    ex, ec = ev.clip_edges(nbits)
    xs, cs = [tx[:16], tx, ex], [tc[:16], tc, ec]
    if nbits == 16:
        nb = ev.neighbours(tx)
        xs.append(nb)
        cs.append(ev.expected_codes(nb, nbits))
    xs.append(tx[-64:])
    cs.append(tc[-64:])
    return np.concatenate(xs), np.concatenate(cs)


def encode_case(nbits, channels):
    """planar rows [channels, frames] with frames % 4 != 0, their interleaved order, the expected payload"""
    x, code = encode_vector(nbits)
    frames = x.size // channels
    while frames % 4 == 0:
        frames -= 1
    x, code = x[-frames * channels:], code[-frames * channels:]
    return np.ascontiguousarray(x.reshape(frames, channels).T), x, ev.codes_to_bytes(code, nbits)


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("nbits", [16, 24, 32])
def test_encode_ties_and_clip_edges(torch_cuda, oracle, nbits, channels):
    planar, inter, want = encode_case(nbits, channels)
    frames = planar.shape[1]
    rows = ru.Rows(channels, frames, 0, 0, torch_cuda).fill(planar)     # 16-byte aligned rows: the tile kernel
    got = d.wav.encode(rows.view, 1, nbits).cpu().numpy()
    assert np.array_equal(np.asarray(oracle.float_to_pcm(inter, nbits)).view(np.uint8).ravel(), want)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, int(bad[0]) // (nbits // 8), inter[int(bad[0]) // (nbits // 8)])
    rows.check_guards()


@pytest.mark.parametrize("nbits", [16, 24, 32])
def test_encode_ties_payload_offset_4(torch_cuda, oracle, nbits):
    """The stereo tile with its payload 4 bytes past a 16-byte boundary (the
    narrowest stores), a guard byte pattern on both sides."""
    torch = torch_cuda
    planar, inter, want = encode_case(nbits, 2)
    frames, poff = planar.shape[1], 4
    rows = ru.Rows(2, frames, 0, 0, torch).fill(planar)
    buf = torch.full((want.size + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    ex = sync_exec(torch)
    assert d.lib().dsp_wav_encode(L.chan_table(rows.ptrs()), 2, frames, 1, nbits, C.c_void_p(buf.data_ptr() + poff),
                                  C.byref(ex)) == 0
    got = buf.cpu().numpy()
    assert np.array_equal(got[poff:poff + want.size], want)
    assert np.all(got[:poff] == 0xA5) and np.all(got[poff + want.size:] == 0xA5)


def test_encode_float_is_a_byte_copy(torch_cuda):
    """format 3: every bit of every special, NaN payload included"""
    s = np.resize(ev.SPECIALS, (3, 1_031))
    for channels in (1, 2, 3):
        rows = ru.Rows(channels, 1_031, 0, 0, torch_cuda).fill(s[:channels])
        got = d.wav.encode(rows.view, 3, 32).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, ev.bits(s[:channels].T).ravel())


# ---------------------------------------------------------------------------
# b. bit-exact families on seeded rows
# ---------------------------------------------------------------------------
def seeded_rows(shape, seed, edges):
    """uniform(-1, 1) rows with SPECIALS at edgevalues.positions of every edge
    in `edges`; each row starts the specials at another one"""
    rng = np.random.default_rng(seed)
    x = rnd(shape, seed)
    Lx = shape[-1]
    pos = np.unique(np.concatenate([ev.positions(Lx, e, rng, 50 if i == 0 else 0) for i, e in enumerate(edges)]))
    for c in range(shape[0]):
        x[c] = ev.seeded(x[c], np.roll(ev.SPECIALS, 7 * c), pos)
    return x


def rows_pair(torch, x, n_out, C_out, off):
    """input rows holding x and output rows, both `off` floats past a 16-byte boundary"""
    return ru.Rows(x.shape[0], x.shape[1], off, 0, torch).fill(x), ru.Rows(C_out, n_out, off, 0, torch)


def done(torch, out):
    torch.cuda.synchronize()
    out.check_output()
    return out.numpy()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("Lx,B", [(10_007, 512), (4_099, 100)])
@pytest.mark.parametrize("pname", list(PLUGINS))
def test_render_offline_specials(torch_cuda, oracle, pname, Lx, B, off):
    x = seeded_rows((2, Lx), Lx, (B, 1024))
    ref = oracle.render_offline([x[0], x[1]], 2, B, SR, oracle.restated_plugin(pname))
    xin, out = rows_pair(torch_cuda, x, ref.shape[1], 2, off)
    d.render_offline(xin.view, 2, B, SR, PLUGINS[pname][0](), out=out.view)
    got = done(torch_cuda, out)
    assert ev.same_bits_nan(got, ref), ev.first_diff(got, ref)
    if pname == "no_op":       # a copy: NaN payloads too
        assert ev.same_bits(got, ref)
    if pname != "IR_test":     # (IR_test ignores its input)
        assert np.isnan(got).any() and np.isinf(got).any() and np.any((got != 0) & (np.abs(got) < ev.FLT_MIN))


@pytest.mark.parametrize("pname", list(PLUGINS))
def test_render_loop_specials(torch_cuda, oracle, pname):
    Lx, B, nb = 5_003, 256, 40          # test_rows_render_loop's shape: the file wraps at the cursor + 3, then every 5003
    x = seeded_rows((3, Lx), 12, (B, 1024))
    ref, cur_ref = oracle.render_loop([x[c] for c in range(3)], 3, B, nb, SR, oracle.restated_plugin(pname),
                                      cursor=Lx - 3)
    xin, out = rows_pair(torch_cuda, x, nb * B, 3, 0)
    _, cur = d.render_loop(xin.view, 3, B, nb, SR, PLUGINS[pname][0](), cursor=Lx - 3, out=out.view)
    got = done(torch_cuda, out)
    assert cur == cur_ref
    assert ev.same_bits_nan(got, ref), ev.first_diff(got, ref)


@pytest.mark.parametrize("pname", ["gain_test", "IR_test"])
def test_render_stft_fused_render_with_specials(torch_cuda, oracle, pname):
    """The fused kernel's render output only: the magnitudes of a frame that
    holds a non-finite sample are not defined."""
    B, Lx = 512, 8192 * 2 + 777
    x = seeded_rows((2, Lx), 31, (B, 4096, 8192))
    ref = oracle.render_offline([x[0], x[1]], 2, B, SR, oracle.restated_plugin(pname))
    out, _ = d.render_stft(dev(torch_cuda, x), 2, B, SR, PLUGINS[pname][0](), window=d.DSP_WIN_HANN)
    torch_cuda.cuda.synchronize()
    got = out.cpu().numpy()
    assert ev.same_bits_nan(got, ref), ev.first_diff(got, ref)


@pytest.mark.parametrize("off", [0, 1])
def test_elementwise_services_specials(torch_cuda, off):
    torch, lib, n = torch_cuda, d.lib(), 4_097
    a = seeded_rows((1, n), 41, (1024,))[0]
    b = ev.seeded(rnd((n,), 42), ev.SPECIALS[::-1], np.arange(3, n, 31))     # other pairings than (s, s)
    b[:ev.SPECIALS.size] = a[:ev.SPECIALS.size] = np.resize(ev.SPECIALS, ev.SPECIALS.size)   # and every (s, s)
    rows = ru.Rows(3, n, off, 0, torch).fill(np.stack([a, b, np.zeros(n, F32)]))
    fp = lambda r: C.cast(C.c_void_p(rows.ptrs()[r]), L.FP)  # noqa: E731
    ex = sync_exec(torch)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        want_gain, want_ip = a * F32(0.37), b * F32(2.0)
        want_mag = np.sqrt((a * a) + (b * b)).astype(F32)

    assert lib.dsp_gain(fp(0), fp(2), 0.37, n, C.byref(ex)) == 0
    got = rows.numpy()[2]
    assert ev.same_bits_nan(got, want_gain), ev.first_diff(got, want_gain)
    assert lib.dsp_magnitude(fp(0), fp(1), fp(2), n, C.byref(ex)) == 0
    got = rows.numpy()[2]
    assert ev.same_bits_nan(got, want_mag), ev.first_diff(got, want_mag)
    assert lib.dsp_copy(fp(0), fp(2), n, C.byref(ex)) == 0
    assert ev.same_bits(rows.numpy()[2], a)
    for v in (-0.0, float(ev.DEN_MIN), float("inf")):
        assert lib.dsp_set(v, fp(2), n, C.byref(ex)) == 0
        assert ev.same_bits(rows.numpy()[2], np.full(n, v, F32)), v
    assert lib.dsp_gain(fp(1), fp(1), 2.0, n, C.byref(ex)) == 0             # in place; overflows FLT_MAX
    got = rows.numpy()[1]
    assert ev.same_bits_nan(got, want_ip), ev.first_diff(got, want_ip)
    assert np.isinf(want_ip[np.abs(b) == ev.FLT_MAX]).all() and np.any(np.abs(b) == ev.FLT_MAX)
    assert ev.same_bits(rows.numpy()[0], a)                                 # the input row is untouched
    rows.check_guards()


@pytest.mark.parametrize("frame0", [0, 1])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_float_wav_decode_moves_bits(torch_cuda, channels, frame0):
    frames = 1_031 + frame0
    s = np.resize(ev.SPECIALS, frames * channels)
    raw = s.view(np.uint8)
    info = wav_info(32, channels, frames, True)
    want = np.ascontiguousarray(s.reshape(frames, channels).T)[:, frame0:]
    got = d.wav.decode(raw, info, frame0, frames - frame0, device="cuda").cpu().numpy()
    assert ev.same_bits(got, want), ev.first_diff(got, want)


def values_equal_zero_sign_free(got, ref):
    """equal as values; where the reference is not zero, in every bit (display.hip header)"""
    nz = ref != 0
    return bool(np.array_equal(got, ref) and np.array_equal(ev.bits(got)[nz], ev.bits(ref)[nz]))


def test_minmax_decimate_specials(torch_cuda, oracle):
    n, P = 10_007, 37
    first = lambda p: (p * n + P - 1) // P  # noqa: E731  (pixel p owns [first(p), first(p + 1)))
    x = (np.random.default_rng(n).standard_normal(n) * 1.5).astype(F32)
    x = ev.seeded(x, ev.SPECIALS[~np.isinf(ev.SPECIALS)], np.arange(11, n, 97))
    x[first(3):first(4)] = np.resize(np.array([-0.0, 0.0], F32), first(4) - first(3))   # only zeros
    x[first(5):first(6)] = ev.QNAN                                                      # only NaN
    x[first(7) + 2], x[first(7) + 130] = np.inf, -np.inf
    x[first(9):first(10)] = np.resize(np.array([ev.QNAN, 0.25, -0.5, ev.DEN_MIN], F32), first(10) - first(9))
    x[first(11):first(12)] = np.resize(np.array([0.0, -0.0, ev.QNAN], F32), first(12) - first(11))
    for off in (0, 1):
        xin = ru.Rows(1, n, off, 0, torch_cuda).fill(x[None])
        vmax, vmin = d.minmax_decimate(xin.view[0], P)
        vmax, vmin = vmax.cpu().numpy(), vmin.cpu().numpy()
        rmax, rmin = oracle.minmax_decimate(x, P)
        assert values_equal_zero_sign_free(vmax, rmax) and values_equal_zero_sign_free(vmin, rmin)
        assert (vmax[3], vmin[3]) == (0.0, 0.0) and (vmax[5], vmin[5]) == (-1.0, 1.0)   # NaN only: the initial values
        assert (vmax[7], vmin[7]) == (np.inf, -np.inf) and (vmax[9], vmin[9]) == (0.25, -0.5)
        assert (vmax[11], vmin[11]) == (0.0, 0.0)
        xin.check_guards()


def test_spectrogram_decimate_specials(torch_cuda, oracle):
    F, K, P = 37, 100, 8
    first = lambda p: (p * F + P - 1) // P  # noqa: E731
    m = np.random.default_rng(F).random((F, K), dtype=F32)
    m[:, 3] = ev.QNAN                                            # NaN only, every pixel: stays 0
    m[:, 5] = np.resize(np.array([-0.0, 0.0], F32), F)           # zeros only
    m[first(2), 7] = np.inf
    m[first(4):first(5), 9] = ev.QNAN
    m[first(4) + 1, 9] = ev.DEN_MIN                              # NaN and one denormal
    m[:, 11] = np.resize(np.array([ev.DEN_MIN, ev.DEN_MAX, ev.FLT_MIN, ev.QNAN], F32), F)
    m[first(6), 13] = ev.FLT_MAX
    got = d.spectrogram_decimate(dev(torch_cuda, m), P).cpu().numpy()
    ref = oracle.spectrogram_decimate(m, P)
    assert values_equal_zero_sign_free(got, ref)
    assert not np.any(got[:, 3]) and not np.any(got[:, 5]) and got[2, 7] == np.inf
    assert ev.bits(got[4, 9]) == ev.bits(ev.DEN_MIN) and got[6, 13] == ev.FLT_MAX


# ---------------------------------------------------------------------------
# c. power-of-two homogeneity
# ---------------------------------------------------------------------------
KS = (-20, 20)
FLOOR = 2.0 ** -60


def sound(*results):
    """the k = 0 results hold no non-zero value below 2^-60 and nothing non-finite"""
    for r in results:
        r = np.asarray(r, np.float64)
        assert np.isfinite(r).all()
        nz = r[r != 0]
        assert nz.size > r.size // 2 and np.min(np.abs(nz)) >= FLOOR, (nz.size, r.size, np.min(np.abs(nz)))


def homogeneous(f, x, power=1):
    """f(2^k x) == 2^(power k) f(x) in every bit, k in KS; f returns a tuple of arrays"""
    base = f(x)
    sound(*base)
    for k in KS:
        got = f((x * F32(2.0 ** k)).astype(F32))
        for g, b in zip(got, base):
            want = (b * b.dtype.type(2.0 ** (power * k))).astype(b.dtype)     # exact: no value leaves the normal range
            assert ev.same_bits(g, want), (k, ev.first_diff(g, want) if b.dtype == F32 else int(np.argmax(g != want)))


def render(torch, plug, C_out, B=512):
    return lambda x: (d.render_offline(dev(torch, x), C_out, B, SR, plug).cpu().numpy(),)


@pytest.mark.parametrize("method,T", [(1, 17), (2, 1_025)])
def test_homogeneity_fir(torch_cuda, method, T):
    """direct form and overlap-save at 3 channels: the pair kernel and the odd channel"""
    x, taps = fir_inputs(T, 6_145)
    homogeneous(render(torch_cuda, d.Plugin.fir(taps, direct=(method == 1)), 3), x)


def test_homogeneity_conv(torch_cuda):
    x, taps = conv_inputs(4_097, 3, 12_289, 4_097)
    homogeneous(render(torch_cuda, d.Plugin.conv(taps), 3), x)


@pytest.mark.parametrize("S", [1, 4])
def test_homogeneity_biquad(torch_cuda, S):
    """B = 1: the render ends with the file, before the response decays below the floor of `sound`"""
    coef, x = biquad_inputs(S, 2 * 2048 + 5)
    homogeneous(render(torch_cuda, d.Plugin.biquad(coef), 3, 1), x)


@pytest.mark.parametrize("sr_in,sr_out", [(48_000, 96_000), (48_000, 11_025)])
def test_homogeneity_resample(torch_cuda, sr_in, sr_out):
    x = rsu.inputs(sr_in + sr_out, 2, 4_097)
    homogeneous(lambda v: (d.resample(dev(torch_cuda, v), sr_in, sr_out).cpu().numpy(),), x)


@pytest.mark.parametrize("n", [1 << 10, 1 << 14])
def test_homogeneity_rfft_irfft(torch_cuda, n):
    x = rnd((2, n - 5), n)          # zero-padded to n
    homogeneous(lambda v: (d.rfft(dev(torch_cuda, v), n).cpu().numpy(),), x)
    spec = d.rfft(dev(torch_cuda, x), n).cpu().numpy()
    homogeneous(lambda s: (d.irfft(dev(torch_cuda, s), n).cpu().numpy(),), spec)


@pytest.mark.parametrize("N,H", [(8192, 4096), (1024, 512)])
def test_homogeneity_stft(torch_cuda, N, H):
    x = rnd((2, 3 * N + 1_234), 21)
    homogeneous(lambda v: (d.stft_magnitude(dev(torch_cuda, v), N=N, H=H, window=d.DSP_WIN_HANN).cpu().numpy(),), x)


def test_homogeneity_render_stft_fused(torch_cuda):
    x = rnd((2, 8192 * 2 + 777), 31)

    def f(v):
        out, mag = d.render_stft(dev(torch_cuda, v), 2, 512, SR, d.Plugin.gain_test(0.2), window=d.DSP_WIN_HANN)
        return out.cpu().numpy()[:, :v.shape[1]], mag.cpu().numpy()     # (the padding past L is zero)

    homogeneous(f, x)


def test_homogeneity_loudness(torch_cuda, oracle):
    """hop energies (2^2k) and both peaks (2^k); the integrated loudness is a logarithm and not bitwise"""
    x = lu.noise(48_000 % 977, 3, 20_003)
    homogeneous(lambda v: (d.loudness(dev(torch_cuda, v), 48_000)["hop_energy"],), x, power=2)
    homogeneous(lambda v: (d.loudness(dev(torch_cuda, v), 48_000)["channel_peaks"],), x)


# ---------------------------------------------------------------------------
# d. quiet and loud frames against float64; the biquad's decaying tail
# ---------------------------------------------------------------------------
SCALES = (-30, -50, -70, -100, 40)
ABS_FLOOR = 2.0 ** -61          # twice the raw square root's flush, 2^-62 (module docstring, dspbench.h)


def assert_frames(mag, ref, what):
    """per frame max|m - ref| <= PEAK_REL_TOL peak + 2^-61, every figure in the message"""
    mag, ref = np.asarray(mag, np.float64), np.asarray(ref, np.float64)
    assert mag.shape == ref.shape and np.isfinite(mag).all(), what
    err, peak = np.abs(mag - ref).max(axis=-1), ref.max(axis=-1)
    bar = PEAK_REL_TOL * peak + ABS_FLOOR
    print(what, "err", err, "peak", peak, "bar", bar)
    assert np.all(err <= bar), (what, err.tolist(), bar.tolist())


@functools.lru_cache(None)
def quiet_input(N, H):
    """3 frames of noise (two hops and a frame) and its float64 magnitudes [F, K]"""
    import oracle
    x = rnd((1, 2 * H + N), N + 3)
    return x, oracle.np_stft_mag(x[0], N, H, oracle.WIN_HANN, N // 2 + 1)


@pytest.mark.parametrize("e", SCALES)
@pytest.mark.parametrize("N,H", [(8192, 4096), (1024, 512)])
def test_stft_quiet_and_loud_frames(torch_cuda, oracle, N, H, e):
    x, ref = quiet_input(N, H)
    assert ref.shape[0] == 3
    xs = (x * F32(2.0 ** e)).astype(F32)     # the reference is taken of xs itself (measured: profiles/stft_quiet_frames.txt)
    ref_e = oracle.np_stft_mag(xs[0], N, H, oracle.WIN_HANN, N // 2 + 1)
    assert np.allclose(ref_e, ref * 2.0 ** e, rtol=1e-6, atol=2.0 ** -140)
    mag = d.stft_magnitude(dev(torch_cuda, xs), N=N, H=H, window=d.DSP_WIN_HANN, K=N // 2 + 1).cpu().numpy()
    assert_frames(mag[0], ref_e, f"stft N={N} 2^{e}")


@pytest.mark.parametrize("e", SCALES)
def test_render_stft_fused_quiet_and_loud_frames(torch_cuda, oracle, e):
    x, _ = quiet_input(8192, 4096)
    xs = np.repeat((x * F32(2.0 ** e)).astype(F32), 2, axis=0)
    out, mag = d.render_stft(dev(torch_cuda, xs), 2, 512, SR, d.Plugin.gain_test(0.2), window=d.DSP_WIN_HANN)
    out, mag = out.cpu().numpy(), mag.cpu().numpy()
    with np.errstate(under="ignore"):
        want = xs * F32(0.2)
    assert ev.same_bits(out, want)
    ref = oracle.np_stft_mag(want[0], 8192, 4096, oracle.WIN_HANN, 4097)
    for c in range(2):
        assert_frames(mag[c], ref, f"render_stft 2^{e} c={c}")


@pytest.mark.parametrize("S", [1, 4])
def test_biquad_impulse_decays_through_denormals(torch_cuda, oracle, S):
    """An impulse into a stable cascade, then zeros for 16,384 samples: the
    float64 response falls below 2^-149.  Within test_gpu_biquad.check's
    bound, finite, and exactly zero where the float64 response is below 2^-160."""
    Ly = 16_384
    for seed in range(64):                       # a cascade whose response dies inside the row
        coef = random_cascade(np.random.default_rng(1000 * S + seed), S)
        x = np.zeros((2, Ly), F32)
        x[:, 0] = 1.0
        y64, _ = oracle.biquad_f64(x[0], coef, Ly)
        dead = np.abs(y64) < 2.0 ** -160
        if np.abs(y64[Ly // 2:]).max() < 2.0 ** -149 and dead[-1024:].all():
            break
    else:
        pytest.fail("no cascade of random_cascade decays below 2^-149 within 8192 samples")
    got = d.render_offline(dev(torch_cuda, x), 2, 512, SR, d.Plugin.biquad(coef)).cpu().numpy()
    assert got.shape == (2, Ly) and np.isfinite(got).all()
    biquad_check(oracle, got, x, coef, Ly)
    # from the first sample after which the float64 response stays below 2^-160
    start = Ly - int(np.argmax(~dead[::-1])) if not dead.all() else 0
    assert start < Ly - 1024
    assert not np.any(got[:, start:]), (start, int(np.flatnonzero(got[0, start:])[0]) + start)


# ---------------------------------------------------------------------------
# e. the second trip of the generic WAV kernels' grid-stride loops
# ---------------------------------------------------------------------------
def test_wav_decode_generic_second_trip(torch_cuda, oracle):
    """4096 blocks x 256 threads x 4 frames = 4,194,304 frames in the first trip"""
    channels, frames = 3, 4_194_304 + 7
    raw = np.random.default_rng(16).integers(0, 256, frames * channels * 2, dtype=np.uint8)
    ref = oracle.deinterleave(oracle.pcm_to_float(raw, 16), channels)
    got = d.wav.decode(raw, wav_info(16, channels, frames), device="cuda")
    torch_cuda.cuda.synchronize()
    got = got.cpu().numpy()
    assert ev.same_bits(got, ref), ev.first_diff(got, ref)


def test_wav_encode_generic_second_trip(torch_cuda, oracle):
    """4096 blocks x 256 threads = 1,048,576 samples in the first trip; 349,526 x 3 = 1,048,578"""
    torch = torch_cuda
    channels, frames, poff = 3, 349_526, 16
    x = (np.random.default_rng(17).random((channels, frames), dtype=F32) * 2.2 - 1.1).astype(F32)
    rows = dev(torch, x)
    nbytes = frames * channels * 2
    buf = torch.full((nbytes + 2 * poff,), 0xA5, dtype=torch.uint8, device="cuda")
    ex = sync_exec(torch)
    ptrs = L.chan_table([rows[c].data_ptr() for c in range(channels)])
    assert d.lib().dsp_wav_encode(ptrs, channels, frames, 1, 16, C.c_void_p(buf.data_ptr() + poff), C.byref(ex)) == 0
    got = buf.cpu().numpy()
    want = np.asarray(oracle.float_to_pcm(np.ascontiguousarray(x.T).ravel(), 16)).view(np.uint8).ravel()
    assert np.array_equal(got[poff:poff + nbytes], want)
    assert np.all(got[:poff] == 0xA5) and np.all(got[poff + nbytes:] == 0xA5)
