"""Every kernel family on rows whose placement the test chooses (rowsutil):
unaligned, strided, mixed in one group, with NaN guards around every row.

The C ABI takes one `float *` per channel and states no alignment; behind it
most kernels pick a vector or a scalar path from the pointers' alignment and
from whether a tile lies inside the row.  Each case runs one call in one
layout and asserts
  a. the bar the kind already has against its reference (constants and
     references imported from the kind's own test module),
  b. the same bits as the `base` layout's result of the same call (alignment
     only changes how words are loaded and stored), except where a docstring
     names the code that legitimately differs,
  c. output guards intact and every output word written,
  d. no non-finite output: the inputs are NaN outside [0, L), and every
     operation here is finite for finite input.
Shapes are the smallest that cross each kernel's tile edge once and leave a
ragged tail.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L
from dspbench.api import _exec
import loudnessutil as lu
import resampleutil as rsu
import rowsutil as ru
import test_gpu_module as tgm
from convutil import conv_f64, conv_inputs
from test_gpu_biquad import check as biquad_check, random_cascade
from test_gpu_conv import check as conv_check
from test_gpu_fir import check_fir
from test_gpu_loudness import LOUD_TOL, ratio as loud_ratio
from test_gpu_parity import PEAK_REL_TOL, PLUGINS, peak_rel_err, rnd
from test_gpu_resample import RESAMPLE_TOL, check as resample_check
from test_gpu_wav import _info as wav_info
from wavutil import samples_bytes

pytestmark = pytest.mark.gpu

SR = 48000.0
_BASE = {}


def in_rows(torch, layout, x, n=None, L_=None):
    io, _, sm = ru.LAYOUTS[layout]
    return ru.Rows(x.shape[0], x.shape[1] if n is None else n, io, sm, torch).fill(x, L_)


def out_rows(torch, layout, Cn, n):
    _, oo, sm = ru.LAYOUTS[layout]
    return ru.Rows(Cn, n, oo, sm, torch)


def vs_base(key, layout, produce):
    """(this layout's result, the base layout's) of produce(layout) -> tuple of arrays"""
    if key not in _BASE:
        _BASE[key] = produce("base")
    return (_BASE[key] if layout == "base" else produce(layout)), _BASE[key]


def finish(torch, out, Ly=None, **kw):
    """(c) and (d) of an output buffer; its rows as a dense host array"""
    if torch is not None:
        torch.cuda.synchronize()
    out.check_output(Ly, **kw)
    y = out.numpy(Ly)
    if not kw:
        ru.assert_finite(y)
    return y


def assert_same_bits(got, base, what=""):
    for g, b in zip(got, base):
        assert ru.same_bits(g, b), (what, int(np.argmax(np.asarray(g).reshape(-1) != np.asarray(b).reshape(-1))))


def render_in(torch, layout, x, Cn, B, plugin, host=False):
    """render_offline of x [Cin, L] into guarded rows -> [Cn, Ly]"""
    t = None if host else torch
    Ly = d.num_blocks(x.shape[1], B) * B
    xin, out = in_rows(t, layout, x), out_rows(t, layout, Cn, Ly)
    y = d.render_offline(xin.view, Cn, B, SR, plugin, out=out.view)
    assert tuple(y.shape) == (Cn, Ly)
    return (finish(torch, out),)


# ---------------------------------------------------------------------------
# built-in render kinds (render.hip): bit-exact against the oracle
# ---------------------------------------------------------------------------
@functools.lru_cache(None)
def render_ref(pname, cin, cout, Lx, B):
    import oracle
    x = rnd((cin, Lx), 11)
    return x, oracle.render_offline([x[c] for c in range(cin)], cout, B, SR, oracle.restated_plugin(pname), L=Lx)


@pytest.mark.parametrize("layout", ru.ALL)
@pytest.mark.parametrize("cin,cout,Lx,B", [(3, 3, 10_007, 512), (2, 3, 4_099, 100)])
@pytest.mark.parametrize("pname", list(PLUGINS))
def test_rows_render_offline(torch_cuda, oracle, pname, cin, cout, Lx, B, layout):
    x, ref = render_ref(pname, cin, cout, Lx, B)
    got, base = vs_base(("render", pname, cin, cout, Lx, B), layout,
                        lambda lay: render_in(torch_cuda, lay, x, cout, B, PLUGINS[pname][0]()))
    assert ru.same_bits(got[0], ref)
    assert_same_bits(got, base)


@functools.lru_cache(None)
def loop_ref(pname):
    import oracle
    Lx, B, nb = 5_003, 256, 40
    x = rnd((3, Lx), 12)
    out, cur = oracle.render_loop([x[c] for c in range(3)], 3, B, nb, SR, oracle.restated_plugin(pname), cursor=Lx - 3)
    return x, out, cur


@pytest.mark.parametrize("layout", ru.ALL)
@pytest.mark.parametrize("pname", list(PLUGINS))
def test_rows_render_loop(torch_cuda, oracle, pname, layout):
    """The file wraps three samples after the cursor and then every 5003: the
    wrap reads neither before the row nor past L (NaN on both sides)."""
    Lx, B, nb = 5_003, 256, 40
    x, ref, cur_ref = loop_ref(pname)

    def produce(lay):
        xin, out = in_rows(torch_cuda, lay, x), out_rows(torch_cuda, lay, 3, nb * B)
        _, cur = d.render_loop(xin.view, 3, B, nb, SR, PLUGINS[pname][0](), cursor=Lx - 3, out=out.view)
        assert cur == cur_ref
        return (finish(torch_cuda, out),)

    got, base = vs_base(("loop", pname), layout, produce)
    assert ru.same_bits(got[0], ref)
    assert_same_bits(got, base)


# ---------------------------------------------------------------------------
# render + STFT, STFT alone
# ---------------------------------------------------------------------------
def even(off):
    return all(o % 2 == 0 for o in ru.offsets(off, 3))


@functools.lru_cache(None)
def render_stft_ref(pname, B, H):
    import oracle
    x, ref = render_ref(pname, 3, 3, 8192 * 2 + 777, B)
    return x, ref, [oracle.np_stft_mag(ref[c], 8192, H, oracle.WIN_HANN, 4097) for c in range(3)]


@pytest.mark.parametrize("layout", ru.FEW)
@pytest.mark.parametrize("H,ld", [(4096, 4097), (4096, 4100), (1000, 4097), (1000, 4100)])
@pytest.mark.parametrize("B", [512, 384])
@pytest.mark.parametrize("pname", ["gain_test", "IR_test"])
def test_rows_render_stft(torch_cuda, oracle, pname, B, H, ld, layout):
    """The render is bit-identical to base in every layout.  The magnitudes
    are only where the call takes base's path: the fused kernel needs
    H % 128 == 0 and every input and output row 8-byte aligned (capi.cpp,
    dsp_render_stft: `fused`), and the render-then-STFT path's 8192-point
    kernel needs 8-byte aligned output rows (capi.cpp stft_device: `fast`);
    a row at an odd float offset takes the two-pass or the generic FFT, whose
    roundings differ (DESIGN: about 1e-8 of the peak).  There only the
    PEAK_REL_TOL bar applies to the magnitudes."""
    K = 4097
    x, ref, mref = render_stft_ref(pname, B, H)
    Lr = ref.shape[1]
    F = d.stft_frames(Lr, 8192, H)
    assert F == mref[0].shape[0] > 1

    def produce(lay):
        xin, out = in_rows(torch_cuda, lay, x), out_rows(torch_cuda, lay, 3, Lr)
        mag = out_rows(torch_cuda, lay, 3, F * ld)
        d.render_stft(xin.view, 3, B, SR, PLUGINS[pname][0](), H=H, K=K, ld=ld, window=d.DSP_WIN_HANN,
                      out=out.view, mag=mag.frames(F, ld))
        y = finish(torch_cuda, out)
        m = finish(torch_cuda, mag, K=K, ld=ld).reshape(3, F, ld)[:, :, :K]   # columns K..ld stay sentinel
        ru.assert_finite(m)
        return y, m

    got, base = vs_base(("render_stft", pname, B, H, ld), layout, produce)
    assert ru.same_bits(got[0], ref)
    assert ru.same_bits(got[0], base[0])
    for c in range(3):
        assert peak_rel_err(got[1][c], mref[c]) <= PEAK_REL_TOL
    io, oo, _ = ru.LAYOUTS[layout]
    if even(oo) and (H % 128 != 0 or even(io)):
        assert ru.same_bits(got[1], base[1])


@functools.lru_cache(None)
def stft_ref(N, H):
    import oracle
    Ls = 3 * N + 1_234
    x = rnd((3, Ls), 21)
    return x, [oracle.np_stft_mag(x[c], N, H, oracle.WIN_HANN, N // 2 + 1) for c in range(3)]


@pytest.mark.parametrize("layout", ru.FEW)
@pytest.mark.parametrize("N,H", [(8192, 4096), (8192, 1000), (1024, 512), (1024, 1000)])
def test_rows_stft_magnitude(torch_cuda, oracle, N, H, layout):
    """The row is longer than L_sig and NaN past it.  N = 8192 with even H
    takes the 8192-point kernel only for 8-byte aligned rows (capi.cpp
    stft_device: `fast`); an odd float offset takes the generic FFT with other
    roundings, so bit-identity with base is asserted where the path is the
    same: every N = 1024 case, and even offsets at N = 8192."""
    K, ld = N // 2 + 1, N // 2 + 4
    x, mref = stft_ref(N, H)
    Ls = x.shape[1]
    F = d.stft_frames(Ls, N, H)

    def produce(lay):
        xin = in_rows(torch_cuda, lay, x, n=Ls + 100)
        mag = out_rows(torch_cuda, lay, 3, F * ld)
        d.stft_magnitude(xin.view, N=N, H=H, window=d.DSP_WIN_HANN, K=K, ld=ld, out=mag.frames(F, ld), L_sig=Ls)
        m = finish(torch_cuda, mag, K=K, ld=ld).reshape(3, F, ld)[:, :, :K]
        ru.assert_finite(m)
        return (m,)

    got, base = vs_base(("stft", N, H), layout, produce)
    for c in range(3):
        assert peak_rel_err(got[0][c], mref[c]) <= PEAK_REL_TOL
    if N != 8192 or even(ru.LAYOUTS[layout][0]):
        assert_same_bits(got, base)


# ---------------------------------------------------------------------------
# FIR (fir.hip, fir_fft.hip), conv (conv_fdl.hip), biquad (iir.hip)
# ---------------------------------------------------------------------------
@functools.lru_cache(None)
def fir_inputs(T, Lx):
    rng = np.random.default_rng(T * 7 + Lx)
    return rng.uniform(-1, 1, (3, Lx)).astype(np.float32), (rng.standard_normal(T) / np.sqrt(T)).astype(np.float32)


# direct form: 17 and 1031 taps; overlap-save (a pair and an odd channel): 64 and 1025
@pytest.mark.parametrize("layout", ru.ALL)
@pytest.mark.parametrize("B", [1, 512])                 # B = 1: odd output rows
@pytest.mark.parametrize("Lx", [14_341, 6_145])         # two 7168-sample frames + 5; two 3072-sample pair hops + 1
@pytest.mark.parametrize("method,T", [(1, 17), (1, 1_031), (2, 64), (2, 1_025)])
def test_rows_fir(torch_cuda, oracle, method, T, Lx, B, layout):
    x, taps = fir_inputs(T, Lx)
    plug = d.Plugin.fir(taps, direct=(method == 1))
    got, base = vs_base(("fir", method, T, Lx, B), layout, lambda lay: render_in(torch_cuda, lay, x, 3, B, plug))
    Ly = d.num_blocks(Lx, B) * B
    for c in range(3):
        check_fir(oracle, got[0][c], x[c], taps, Ly, method)
    assert_same_bits(got, base)


@pytest.mark.parametrize("layout", ru.ALL)
@pytest.mark.parametrize("B", [1, 512])
@pytest.mark.parametrize("T", [4_097, 8_193])           # two and three partitions of 4096
def test_rows_conv(torch_cuda, T, B, layout):
    Lx = 12_289                                         # three 4096-sample frames + 1
    x, taps = conv_inputs(T, 3, Lx, T)
    got, base = vs_base(("conv", T, B), layout, lambda lay: render_in(torch_cuda, lay, x, 3, B, d.Plugin.conv(taps)))
    Ly = d.num_blocks(Lx, B) * B
    for c in range(3):
        conv_check(got[0][c], conv_f64(x[c], taps, Ly), f"T={T} B={B} {layout} c={c}")
    assert_same_bits(got, base)


@functools.lru_cache(None)
def biquad_inputs(S, Lx):
    rng = np.random.default_rng(1000 * S + Lx)
    return random_cascade(rng, S), rng.uniform(-1, 1, (3, Lx)).astype(np.float32)


@pytest.mark.parametrize("layout", ru.ALL)
@pytest.mark.parametrize("in_ch", [3, 2])
@pytest.mark.parametrize("B", [1, 256])
@pytest.mark.parametrize("Lx", [2 * 2048 + 5, 2_047])   # two tiles and a ragged third; less than one
@pytest.mark.parametrize("S", [1, 4])                   # one channel per wave; channel pairs
def test_rows_biquad(torch_cuda, oracle, S, Lx, B, in_ch, layout):
    coef, x3 = biquad_inputs(S, Lx)
    x = x3[:in_ch]
    got, base = vs_base(("biquad", S, Lx, B, in_ch), layout,
                        lambda lay: render_in(torch_cuda, lay, x, 3, B, d.Plugin.biquad(coef)))
    biquad_check(oracle, got[0], x, coef, d.num_blocks(Lx, B) * B)
    assert_same_bits(got, base)


# ---------------------------------------------------------------------------
# resample (resample.hip), loudness (loudness.hip)
# ---------------------------------------------------------------------------
# resample_blocking (resample.hip): 2/1 stages tiles of 1024 periods in LDS
# (resample_phase_kernel: 4 full tiles of 2048 outputs and a ragged one at
# L = 4097); 147/640 needs 64 * 640 + S floats of LDS, above the CU's 160 KB
# (resample_direct_kernel).  No pair of test_gpu_resample.RATES takes the
# direct kernel, so its pair is the standard-rate one below.
RS_RATES = [(48_000, 96_000), (48_000, 11_025)]


def resample_in(torch, layout, x, sr_in, sr_out, zeros, host=False):
    t = None if host else torch
    lout = rsu.plan(sr_in, sr_out, x.shape[1], zeros=zeros)["Lout"]
    xin, out = in_rows(t, layout, x), out_rows(t, layout, x.shape[0], lout)
    y = d.resample(xin.view, sr_in, sr_out, zeros=zeros, out=out.view)
    assert tuple(y.shape) == (x.shape[0], lout)
    return (finish(torch, out),)


@functools.lru_cache(None)
def resample_ref(sr_in, sr_out, zeros, Lx):
    x = rsu.inputs(sr_in + zeros + Lx, 2, Lx)
    return x, [rsu.resample_f64(x[c], sr_in, sr_out, zeros=zeros) for c in range(2)]


@pytest.mark.parametrize("layout", ru.ALL)
@pytest.mark.parametrize("Lx", [4_097, 300])
@pytest.mark.parametrize("zeros", [4, 64])
@pytest.mark.parametrize("sr_in,sr_out", RS_RATES)
def test_rows_resample(torch_cuda, sr_in, sr_out, zeros, Lx, layout):
    x, y64 = resample_ref(sr_in, sr_out, zeros, Lx)
    got, base = vs_base(("resample", sr_in, sr_out, zeros, Lx), layout,
                        lambda lay: resample_in(torch_cuda, lay, x, sr_in, sr_out, zeros))
    for c in range(2):
        resample_check(got[0][c], y64[c], f"{sr_in}->{sr_out} Z={zeros} L={Lx} {layout} c={c}")
    assert_same_bits(got, base)


LOUD_KEYS = ("integrated", "range", "momentary_max", "short_term_max", "sample_peak", "true_peak", "blocks",
             "gated_blocks")


def loudness_in(torch, layout, x, sr, host=False):
    xin = in_rows(None if host else torch, layout, x)
    r = d.loudness(xin.view, sr)
    if not host:
        torch.cuda.synchronize()
    res = np.array([r[k] for k in LOUD_KEYS], np.float64)
    # (short_term_max is -inf by definition below 3 s of signal, and the range 0)
    ru.assert_finite(r["hop_energy"], r["channel_peaks"], res[[0, 2, 4, 5]])
    return r["hop_energy"], r["channel_peaks"], res


@functools.lru_cache(None)
def loudness_ref(sr):
    import oracle  # noqa: F401  (loudnessutil's float64 cascade)
    Lx = 20_003
    x = lu.noise(sr % 977, 3, Lx)
    ovs = lu.plan(sr)["oversample"]
    return (x, [lu.hop_energy64(x[c], sr) for c in range(3)],
            [float(np.max(np.abs(rsu.resample_f64(x[c], sr, ovs * sr)))) for c in range(3)])


@pytest.mark.parametrize("layout", ru.FEW)
@pytest.mark.parametrize("sr", [48_000, 44_100])
def test_rows_loudness(torch_cuda, oracle, sr, layout):
    """Inputs only: the true-peak kernel reads half - 1 samples around both
    ends of the row, which are NaN here."""
    x, z64, tp64 = loudness_ref(sr)
    got, base = vs_base(("loudness", sr), layout, lambda lay: loudness_in(torch_cuda, lay, x, sr))
    z, peaks, _ = got
    assert z.shape == (3, 20_003 // lu.plan(sr)["hop"])
    for c in range(3):
        assert loud_ratio(z[c], z64[c]) <= LOUD_TOL
        assert peaks[c, 0] == float(np.max(np.abs(x[c])))
        assert abs(peaks[c, 1] - tp64[c]) <= RESAMPLE_TOL * tp64[c]
    assert_same_bits(got, base)


# ---------------------------------------------------------------------------
# GENERIC plugins (plugin_driver.inl, plugin_driver_seg.inl)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ru.FEW)
def test_rows_generic_stateless_plugin(torch_cuda, oracle, layout):
    """gain_test.cpp compiled unchanged, not specialised: the LDS-blocks driver's copies."""
    name, Lx, B = "gain_test", 10_007, 512
    if not tgm.have(name):
        pytest.skip("oracle/_ref not built")
    mod = tgm.load(name)
    params = mod.default_parameters()
    mod.initialize_state(params, 3, SR)
    x = rnd((3, Lx), 13)
    want = oracle.render_offline([x[c] for c in range(3)], 3, B, SR, oracle.RefPlugin(name, 3, SR).as_oracle())
    got, base = vs_base(("plugin", name), layout,
                        lambda lay: render_in(torch_cuda, lay, x, 3, B, mod.plugin(params, name, specialize=False)))
    assert ru.same_bits(got[0], want)
    assert_same_bits(got, base)


@pytest.mark.parametrize("layout", ru.FEW)
def test_rows_generic_biquad_plugin(torch_cuda, oracle, layout):
    """plugins/biquad.cpp compiled unchanged (the segment driver): bit-exact
    against the serial fp32 chain, as test_biquad_source_plugin_serial_and_kind."""
    import struct
    co = os.path.join(tgm.MODS, "mod_biquad.co")
    if not os.path.exists(co):
        pytest.skip("modules not built")
    Lx, B = 10_007, 512
    mod = tgm.load("biquad")
    params = mod.default_parameters()
    x = rnd((3, Lx), 14)

    def produce(lay):
        mod.initialize_state(params, 3, SR)   # the State persists across renders
        return render_in(torch_cuda, lay, x, 3, B, mod.plugin(params))

    got, base = vs_base(("plugin", "biquad"), layout, produce)
    mod.initialize_state(params, 3, SR)
    coef = np.array([struct.unpack("<5f", mod.read_state()[:20])], np.float32)
    for c in range(3):
        assert ru.same_bits(got[0][c], oracle.biquad_f32(x[c], coef, got[0].shape[1]))
    assert_same_bits(got, base)


# ---------------------------------------------------------------------------
# WAV decode (wav.hip), display reductions (display.hip)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ru.FEW)
@pytest.mark.parametrize("bits,channels", [(16, 2), (24, 3)])
def test_rows_wav_decode(torch_cuda, oracle, bits, channels, layout):
    frames = 5_003
    raw = samples_bytes(np.random.default_rng(bits), frames * channels, bits, False)
    ref = oracle.deinterleave(oracle.pcm_to_float(raw, bits, False), channels)
    info = wav_info(bits, channels, frames)
    data = torch_cuda.from_numpy(np.ascontiguousarray(raw)).cuda()

    def produce(lay):
        out = out_rows(torch_cuda, lay, channels, frames)
        ex = _exec(out.view)
        L.check(L.lib().dsp_wav_decode(C.c_void_p(data.data_ptr()), C.byref(info), 0, frames, L.chan_table(out.ptrs()),
                                       C.byref(ex)), "dsp_wav_decode")
        return (finish(torch_cuda, out),)

    got, base = vs_base(("wav", bits, channels), layout, produce)
    assert ru.same_bits(got[0], ref)
    assert_same_bits(got, base)


def test_rows_minmax_decimate(torch_cuda, oracle):
    n, P = 10_007, 37
    x = (np.random.default_rng(n).standard_normal((1, n)) * 1.5).astype(np.float32)
    xin = ru.Rows(1, n, 1, 0, torch_cuda).fill(x)
    assert xin.ptrs()[0] % 16 == 4
    vmax, vmin = d.minmax_decimate(xin.view[0], P)
    vmax, vmin = vmax.cpu().numpy(), vmin.cpu().numpy()
    ru.assert_finite(vmax, vmin)
    rmax, rmin = oracle.minmax_decimate(x[0], P)
    assert ru.same_bits(vmax, rmax) and ru.same_bits(vmin, rmin)
    xin.check_guards()    # an input: nothing around it is written


def test_rows_spectrogram_decimate(torch_cuda, oracle):
    F, K, ld, P = 37, 100, 103, 8
    m = np.random.default_rng(F).random((F, K), dtype=np.float32)
    buf = ru.Rows(1, F * ld, 1, 0, torch_cuda)
    mag = buf.frames(F, ld)[0][:, :K]
    mag.copy_(torch_cuda.from_numpy(m).cuda())   # columns K..ld and the guards stay NaN
    assert mag.data_ptr() % 16 == 4 and mag.stride(0) == ld
    got = d.spectrogram_decimate(mag, P).cpu().numpy()
    ru.assert_finite(got)
    assert ru.same_bits(got, oracle.spectrogram_decimate(m, P))
    buf.check_guards(F * ld, K=K, ld=ld)


# ---------------------------------------------------------------------------
# host buffers: the staging layer takes row pointers, not one block
# ---------------------------------------------------------------------------
HOST = ("odd_stride", "in1")


@pytest.mark.parametrize("layout", HOST)
def test_rows_host_render(torch_cuda, oracle, layout):
    x, ref = render_ref("gain_test", 3, 3, 10_007, 512)
    got = render_in(torch_cuda, layout, x, 3, 512, PLUGINS["gain_test"][0](), host=True)
    assert ru.same_bits(got[0], ref)


@pytest.mark.parametrize("layout", HOST)
def test_rows_host_conv(torch_cuda, layout):
    T, Lx, B = 4_097, 12_289, 512
    x, taps = conv_inputs(T, 3, Lx, T)
    _, base = vs_base(("conv", T, B), "base", lambda lay: render_in(torch_cuda, lay, x, 3, B, d.Plugin.conv(taps)))
    host = render_in(torch_cuda, layout, x, 3, B, d.Plugin.conv(taps), host=True)
    for c in range(3):
        conv_check(host[0][c], conv_f64(x[c], taps, host[0].shape[1]), f"host {layout} c={c}")
    assert_same_bits(host, base)


@pytest.mark.parametrize("layout", HOST)
def test_rows_host_resample(torch_cuda, layout):
    sr_in, sr_out, zeros, Lx = 48_000, 96_000, 64, 4_097
    x, y64 = resample_ref(sr_in, sr_out, zeros, Lx)
    _, base = vs_base(("resample", sr_in, sr_out, zeros, Lx), "base",
                      lambda lay: resample_in(torch_cuda, lay, x, sr_in, sr_out, zeros))
    host = resample_in(torch_cuda, layout, x, sr_in, sr_out, zeros, host=True)
    for c in range(2):
        resample_check(host[0][c], y64[c], f"host {layout} c={c}")
    assert_same_bits(host, base)


@pytest.mark.parametrize("layout", HOST)
def test_rows_host_loudness(torch_cuda, oracle, layout):
    sr = 48_000
    x, z64, _ = loudness_ref(sr)
    _, base = vs_base(("loudness", sr), "base", lambda lay: loudness_in(torch_cuda, lay, x, sr))
    host = loudness_in(torch_cuda, layout, x, sr, host=True)
    for c in range(3):
        assert loud_ratio(host[0][c], z64[c]) <= LOUD_TOL
    assert_same_bits(host, base)
