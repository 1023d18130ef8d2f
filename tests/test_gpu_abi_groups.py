"""The C ABI's channel groups and host-buffer staging (csrc/capi_impl.hpp, csrc/capi_render.cpp).

Kernels take at most 16 row pointers, so every entry point walks its rows in
groups of 16 (and FIR / BIQUAD split a group into pairs and an odd last
channel).  These tests run each entry point with more than 16 rows: C = 19
output rows (one full group, then a pair and an odd last channel) over a
17-channel file (the last two rows have no file), rows of distinct noise so
that a misrouted pointer shows.  Expected values and bounds are the ones the
single-group tests use (test_gpu_parity, test_gpu_fir, test_gpu_biquad): the
oracle or float64, never a second call into the library.

The second half is DSP_EXEC_HOST_BUFFERS: a call on numpy arrays is staged
through device buffers by the library and equals the call on device tensors
bit for bit, every output included.
"""
import ctypes as C

import numpy as np
import pytest

import dspbench as d
from test_gpu_biquad import check as check_biquad, rbj
from test_gpu_fir import check_fir
from test_gpu_parity import PEAK_REL_TOL, PLUGINS, oracle_plugin, peak_rel_err, rnd, to_dev

pytestmark = pytest.mark.gpu

NC, NIN = 19, 17


def dev_rows(torch, x):
    """x [C, L] on the device with a row stride that is a multiple of 4 floats:
    every row 16-byte aligned whatever L is (the vector and fused paths)."""
    c, n = x.shape
    t = torch.zeros((c, (n + 3) // 4 * 4), dtype=torch.float32, device="cuda")
    t[:, :n] = torch.from_numpy(np.ascontiguousarray(x))
    return t[:, :n]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- more than 16 channels --------------------------------------------------

@pytest.mark.parametrize("pname", ["gain_test", "no_op", "IR_test"])
@pytest.mark.parametrize("cin", [NIN, 0, 21])
def test_groups_render_offline(torch_cuda, oracle, pname, cin):
    L, B = 1000, 128
    x = rnd((max(cin, 1), L), 101)[:cin]
    ref = oracle.render_offline([x[c] for c in range(cin)], NC, B, 48000.0, oracle_plugin(oracle, pname), L=L)
    got = d.render_offline(to_dev(torch_cuda, x) if cin else None, NC, B, 48000.0, PLUGINS[pname][0](), L_file=L,
                           out=torch_cuda.empty((NC, d.num_blocks(L, B) * B), device="cuda")).cpu().numpy()
    assert bits_equal(got, ref), f"max abs diff {np.max(np.abs(got - ref))}"


@pytest.mark.parametrize("method", [2, 1], ids=["ols", "direct"])
def test_groups_render_offline_fir(torch_cuda, oracle, method):
    L, B, T = 10_000, 512, 64
    rng = np.random.default_rng(102)
    x = rng.uniform(-1, 1, (NIN, L)).astype(np.float32)
    taps = (rng.standard_normal(T) / np.sqrt(T)).astype(np.float32)
    out = d.render_offline(to_dev(torch_cuda, x), NC, B, 48000.0, d.Plugin.fir(taps, direct=(method == 1)))
    out = out.cpu().numpy()
    Ly = d.num_blocks(L, B) * B
    assert out.shape == (NC, Ly)
    for c in range(NIN):
        check_fir(oracle, out[c], x[c], taps, Ly, method)
    assert not out[NIN:].any()  # rows the file lacks: exact zeros


@pytest.mark.parametrize("S", [1, 2], ids=["single", "pairs"])
def test_groups_render_offline_biquad(torch_cuda, oracle, S):
    L, B = 20_000, 512
    coef = np.array([rbj("hp", 300.0, 0.9), rbj("lp", 4000.0, 1.2)][:S], np.float32)
    x = np.random.default_rng(103 + S).uniform(-1, 1, (NIN, L)).astype(np.float32)
    got = d.render_offline(to_dev(torch_cuda, x), NC, B, 48000.0, d.Plugin.biquad(coef)).cpu().numpy()
    assert got.shape == (NC, d.num_blocks(L, B) * B)
    check_biquad(oracle, got, x, coef, got.shape[1])
    assert not got[NIN:].any()  # zero input from zero state


@pytest.mark.parametrize("N,H", [(8192, 4096), (1024, 512)])
def test_groups_stft_magnitude(torch_cuda, oracle, N, H):
    Cs, L = 17, 8192 * 2 + 100
    x = rnd((Cs, L), 104)
    mag = d.stft_magnitude(dev_rows(torch_cuda, x), N=N, H=H, window=d.DSP_WIN_HANN).cpu().numpy()
    for c in range(Cs):
        ref = oracle.np_stft_mag(x[c], N, H, d.DSP_WIN_HANN, N // 2 + 1)
        assert mag[c].shape == ref.shape
        assert peak_rel_err(mag[c], ref) <= PEAK_REL_TOL, c


FUSED = dict(L=8192 * 2 + 777, N=8192, H=4096, K=4097, C=18, cin=17)


def fused_call(torch, pname, B, x):
    return d.render_stft(dev_rows(torch, x), FUSED["C"], B, 48000.0, PLUGINS[pname][0](), N=FUSED["N"],
                         H=FUSED["H"], window=d.DSP_WIN_HANN)


@pytest.mark.parametrize("pname,B", [("IR_test", 512), ("gain_test", 512), ("IR_test", 384), ("gain_test", 384)])
def test_groups_render_stft_fused(torch_cuda, oracle, pname, B):
    """B = 512 with IR_test: the launch that also renders the tail; the other
    three: the tail [F H, Lr) goes through the render kernel, group by group."""
    Cn, cin = FUSED["C"], FUSED["cin"]
    x = rnd((cin, FUSED["L"]), 105)
    out, mag = fused_call(torch_cuda, pname, B, x)
    out, mag = out.cpu().numpy(), mag.cpu().numpy()
    ref = oracle.render_offline([x[c] for c in range(cin)], Cn, B, 48000.0, oracle_plugin(oracle, pname))
    assert bits_equal(out, ref)
    for c in range(Cn):
        mref = oracle.np_stft_mag(ref[c], 8192, 4096, d.DSP_WIN_HANN, 4097)
        assert mag[c].shape == mref.shape
        assert peak_rel_err(mag[c], mref) <= PEAK_REL_TOL, c


def test_groups_render_stft_fused_timing_records(torch_cuda):
    """One timing record per group of 16 rows, each with the fused launch's
    algorithmic bytes: render write + magnitudes + the tail the launch renders
    itself, and no file read for IR_test (its map ignores the input)."""
    lib = d.lib()
    Cn, B, H, K = FUSED["C"], 512, FUSED["H"], FUSED["K"]
    x = rnd((FUSED["cin"], FUSED["L"]), 105)
    Lr = d.num_blocks(FUSED["L"], B) * B
    F = d.stft_frames(Lr, FUSED["N"], H)
    assert F == 3 and Lr > F * H
    lib.dsp_kernel_timing(None, None, None)
    lib.dsp_kernel_timing_enable(1)
    try:
        fused_call(torch_cuda, "IR_test", B, x)
        torch_cuda.cuda.synchronize()
    finally:
        lib.dsp_kernel_timing_enable(0)
    ms, n, nbytes = C.c_double(), C.c_uint64(), C.c_uint64()
    assert lib.dsp_kernel_timing(C.byref(ms), C.byref(n), C.byref(nbytes)) == 0
    want = sum(cn * F * H * 4 + cn * F * K * 4 + cn * (Lr - F * H) * 4 for cn in (16, Cn - 16))
    assert n.value == 2
    assert nbytes.value == want, (nbytes.value, want)


def test_groups_render_loop(torch_cuda, oracle):
    Cn, cin, L, B, nb, cursor = 18, 17, 1000, 128, 5, 700
    x = rnd((cin, L), 106)
    ref, ref_cur = oracle.render_loop([x[c] for c in range(cin)], Cn, B, nb, 48000.0,
                                      oracle_plugin(oracle, "gain_test"), cursor=cursor)
    got, cur = d.render_loop(to_dev(torch_cuda, x), Cn, B, nb, 48000.0, PLUGINS["gain_test"][0](), cursor=cursor)
    assert cur == ref_cur == (cursor + nb * B) % L
    assert bits_equal(got.cpu().numpy(), ref)
    # FIR loops over the materialised wrapped file (the whole wrapped stream
    # convolved: test_render_loop_generic_and_fir's bound)
    taps = rnd((1, 8), 107)[0] * 0.3
    got, cur = d.render_loop(to_dev(torch_cuda, x), Cn, B, nb, 48000.0, d.Plugin.fir(taps), cursor=cursor)
    got = got.cpu().numpy()
    assert cur == ref_cur
    idx = (cursor + np.arange(nb * B)) % L
    for c in range(cin):
        want = oracle.fir_f64(x[c][idx], taps)
        assert np.max(np.abs(got[c].astype(np.float64) - want[: nb * B])) <= 2e-6 * np.max(np.abs(want)), c
    assert not got[cin:].any()


@pytest.mark.parametrize("ir_len", [2048, 256])
def test_groups_ir_analysis(torch_cuda, oracle, ir_len):
    Cs = 17
    ir, mag = d.ir_analysis(d.Plugin.gain_test(0.2), Cs, 48000.0, ir_len=ir_len, device="cuda")
    ir, mag = ir.cpu().numpy(), mag.cpu().numpy()
    expect = np.zeros((Cs, ir_len), np.float32)
    expect[:, 0] = np.float32(1.0) * np.float32(0.2)
    assert bits_equal(ir, expect)
    ref = oracle.np_ir_magnitude(expect[0], ir_len)  # flat: (float)0.2 * w[0] / sqrt(4 ir_len), w[0] = 0.08
    flat = float(np.float32(0.2)) * 0.08 / np.sqrt(4 * ir_len)
    assert np.max(np.abs(ref - flat)) <= 1e-12 * flat
    assert np.max(np.abs(mag - ref)) <= 1e-6 * flat * 8  # test_ir_analysis_gain_flat's bar


# ---- host buffers -------------------------------------------------------------

@pytest.mark.parametrize("Cn", [2, 17])
def test_host_render_offline(torch_cuda, Cn):
    x = rnd((Cn, 3000), 201)
    dev = d.render_offline(to_dev(torch_cuda, x), Cn, 128, 48000.0, d.Plugin.gain_test(0.3)).cpu().numpy()
    host = d.render_offline(x, Cn, 128, 48000.0, d.Plugin.gain_test(0.3))
    assert dev.shape == (Cn, 3072) and bits_equal(host, dev)


@pytest.mark.parametrize("N,H,L", [(8192, 4096, 8192 + 4096 + 100), (8192, 4096, 5000), (256, 128, 1000),
                                   (256, 128, 200)])
def test_host_stft_magnitude(torch_cuda, N, H, L):
    """L < N: no frame, nothing copied back."""
    x = rnd((2, L), 202)
    dev = d.stft_magnitude(dev_rows(torch_cuda, x), N=N, H=H).cpu().numpy()
    host = d.stft_magnitude(x, N=N, H=H)
    assert dev.shape == (2, d.stft_frames(L, N, H), N // 2 + 1) and bits_equal(host, dev)


@pytest.mark.parametrize("pname,B,L", [("IR_test", 512, 8192 * 2 + 300), ("gain_test", 100, 8192 + 3000)])
def test_host_render_stft(torch_cuda, pname, B, L):
    x = rnd((2, L), 203)
    dout, dmag = d.render_stft(dev_rows(torch_cuda, x), 2, B, 48000.0, PLUGINS[pname][0]())
    hout, hmag = d.render_stft(x, 2, B, 48000.0, PLUGINS[pname][0]())
    assert dmag.shape[1] >= 1
    assert bits_equal(hout, dout.cpu().numpy()) and bits_equal(hmag, dmag.cpu().numpy())


def test_host_ir_analysis(torch_cuda):
    dir_, dmag = d.ir_analysis(d.Plugin.ir_test(0.9, 0.002), 2, 48000.0, device="cuda")
    hir, hmag = d.ir_analysis(d.Plugin.ir_test(0.9, 0.002), 2, 48000.0)
    assert bits_equal(hir, dir_.cpu().numpy()) and bits_equal(hmag, dmag.cpu().numpy())


def test_host_fft_services(torch_cuda):
    x = rnd((64,), 204)
    dre, dim = d.fft_forward(to_dev(torch_cuda, x))
    hre, him = d.fft_forward(x)
    assert bits_equal(hre, dre.cpu().numpy()) and bits_equal(him, dim.cpu().numpy())
    dback = d.fft_reverse(dre, dim)
    assert bits_equal(d.fft_reverse(hre, him), dback.cpu().numpy())


@pytest.mark.parametrize("n", [0, 5000])
def test_host_minmax_decimate(torch_cuda, n):
    x = rnd((n,), 205)
    dmax, dmin = d.minmax_decimate(to_dev(torch_cuda, x), 37)
    hmax, hmin = d.minmax_decimate(x, 37)
    assert hmax.shape == (37,)
    assert bits_equal(hmax, dmax.cpu().numpy()) and bits_equal(hmin, dmin.cpu().numpy())


def test_host_spectrogram_decimate(torch_cuda):
    F, K, ld = 50, 33, 40
    wide = np.abs(rnd((F, ld), 206))
    dev = d.spectrogram_decimate(to_dev(torch_cuda, wide)[:, :K], 7).cpu().numpy()
    host = d.spectrogram_decimate(wide[:, :K], 7)
    assert dev.shape == (7, K) and bits_equal(host, dev)
