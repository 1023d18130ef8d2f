"""DSP_PLUGIN_CONV on the GPU (csrc/conv_fdl.hip): convolution with a long
impulse response by partitioned FFT overlap-save, against the float64 FFT
convolution (convutil.conv_f64, pinned to the oracle in test_conv_plan.py).

Signals: x uniform in [-1, 1], taps randn(T) / sqrt(T).

Tolerance: max |y - y64| <= CONV_TOL * max |y64| per channel, the form
test_gpu_fir.py's OLS_TOL has.  CONV_TOL is 4 x the larger of two measured
worst ratios over these shapes (1 .. 64 partitions):
  tools/conv_model.py (the same partition arithmetic in float32, torch.fft on
      the CPU):                                                   2.31e-07
  the GPU (this file's cases, MI355X):                            5.96e-07
The margin absorbs other summation orders (the error grows roughly with the
square root of the partitions; both measurements include the 64-partition
case).  An indexing mistake is an error of order 1.  One constant serves: it is
below 10 x OLS_TOL = 2e-5.
"""
import numpy as np
import pytest

import dspbench as d
from convutil import conv_f64, conv_inputs

pytestmark = pytest.mark.gpu

CONV_TOL = 4 * 5.96e-07  # = 2.4e-6


def ratio(y, y64):
    return float(np.max(np.abs(np.asarray(y, np.float64) - y64)) / max(float(np.max(np.abs(y64))), 1e-30))


def check(y, y64, what):
    r = ratio(y, y64)
    print(f"conv ratio {what}: {r:.3e}")
    assert r <= CONV_TOL, (what, r)


def render(torch, x, C, B, taps, **kw):
    out = d.render_offline(torch.from_numpy(x).cuda() if x is not None else None, C, B, 48000.0,
                           d.Plugin.conv(taps), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# every T with every L; B cycles so that each value meets each L and T somewhere
SHAPES = [(T, Lx, (512, 100, 1)[(i + j) % 3])
          for i, T in enumerate((2049, 4096, 4097, 8193, 40_000, 70_001))
          for j, Lx in enumerate((100, 4096, 4097, 12_289, 70_001))]


@pytest.mark.parametrize("T,Lx,B", SHAPES)
def test_gpu_conv_shapes(torch_cuda, T, Lx, B):
    x, taps = conv_inputs(T + Lx, 1, Lx, T)
    y = render(torch_cuda, x, 1, B, taps)
    Ly = -(-Lx // B) * B
    assert y.shape == (1, Ly)
    check(y[0], conv_f64(x[0], taps, Ly), f"T={T} L={Lx} B={B}")


@pytest.mark.parametrize("dly", [0, 4095, 4096, 4097, 12_288])
def test_gpu_conv_unit_impulse_is_a_delay(torch_cuda, dly):
    T, Lx = 12_289, 12_289
    x, _ = conv_inputs(dly, 1, Lx, 1)
    taps = np.zeros(T, np.float32)
    taps[dly] = 1.0
    y = render(torch_cuda, x, 1, 512, taps)
    want = np.zeros(y.shape[1])
    want[dly:dly + Lx] = x[0][:want.size - dly]
    check(y[0], want, f"delay {dly}")


@pytest.mark.parametrize("C,in_ch", [(1, 1), (2, 2), (3, 3), (5, 4), (17, 17)])
def test_gpu_conv_channels(torch_cuda, C, in_ch):
    Lx, T, B = 12_289, 8193, 512
    x, taps = conv_inputs(C, in_ch, Lx, T)
    y = render(torch_cuda, x, C, B, taps)
    Ly = -(-Lx // B) * B
    for c in range(C):
        if c < in_ch:
            check(y[c], conv_f64(x[c], taps, Ly), f"C={C} c={c}")
        else:
            assert not y[c].any()


def test_gpu_conv_no_input_channels_is_silence(torch_cuda):
    out = torch_cuda.full((2, 5120), 7.0, dtype=torch_cuda.float32, device="cuda")
    d.render_offline(None, 2, 512, 48000.0, d.Plugin.conv(np.ones(5000, np.float32)), out=out, L_file=5000)
    torch_cuda.cuda.synchronize()
    assert not out.cpu().numpy().any()


def test_gpu_conv_host_buffers_cache_hit_and_interleaving(torch_cuda):
    Lx, B = 12_289, 100
    x, ta = conv_inputs(1, 2, Lx, 5000)
    _, tb = conv_inputs(2, 2, Lx, 9000)
    a1 = render(torch_cuda, x, 2, B, ta)
    b1 = render(torch_cuda, x, 2, B, tb)
    a2 = render(torch_cuda, x, 2, B, ta)      # the cached table
    b2 = render(torch_cuda, x, 2, B, tb)
    assert np.array_equal(a1, a2) and np.array_equal(b1, b2) and not np.array_equal(a1, b1)
    host = d.render_offline(x, 2, B, 48000.0, d.Plugin.conv(ta))
    assert isinstance(host, np.ndarray) and np.array_equal(host, a1)
    Ly = a1.shape[1]
    check(a1[1], conv_f64(x[1], ta, Ly), "taps a")
    check(b1[1], conv_f64(x[1], tb, Ly), "taps b")


def test_gpu_conv_render_stft(torch_cuda, oracle):
    Lx, B = 70_001, 512
    x, taps = conv_inputs(3, 2, Lx, 6000)
    out, mag = d.render_stft(torch_cuda.from_numpy(x).cuda(), 2, B, 48000.0, d.Plugin.conv(taps),
                             window=d.DSP_WIN_HANN)
    torch_cuda.cuda.synchronize()
    out, mag = out.cpu().numpy(), mag.cpu().numpy()
    assert np.array_equal(out, render(torch_cuda, x, 2, B, taps))
    assert mag.shape[1] == d.stft_frames(out.shape[1], 8192, 4096) > 0
    for c in range(2):
        mref = oracle.np_stft_mag(out[c], 8192, 4096, oracle.WIN_HANN, 4097)
        assert np.max(np.abs(mag[c] - mref).max(axis=1) / mref.max(axis=1)) <= 1e-6


def test_gpu_conv_ir_analysis(torch_cuda):
    _, taps = conv_inputs(4, 1, 1, 5000)
    ir, _ = d.ir_analysis(d.Plugin.conv(taps), 2, 48000.0, 2048, device="cuda")
    torch_cuda.cuda.synchronize()
    ir = ir.cpu().numpy()
    for c in range(2):
        check(ir[c], taps[:2048].astype(np.float64), f"ir c={c}")


def test_gpu_conv_render_loop(torch_cuda):
    Lx, B, nb, cursor = 5000, 512, 40, 1234
    x, taps = conv_inputs(5, 2, Lx, 6000)
    out, cur = d.render_loop(torch_cuda.from_numpy(x).cuda(), 2, B, nb, 48000.0, d.Plugin.conv(taps), cursor=cursor)
    torch_cuda.cuda.synchronize()
    out = out.cpu().numpy()
    assert cur == (cursor + nb * B) % Lx
    idx = (cursor + np.arange(nb * B)) % Lx
    for c in range(2):
        check(out[c], conv_f64(x[c][idx], taps, nb * B), f"loop c={c}")


def test_gpu_conv_refusals(torch_cuda):
    x, taps = conv_inputs(6, 1, 8192, 5000)
    xd = torch_cuda.from_numpy(x).cuda()
    with pytest.raises(d.DspError):   # in place
        d.render_offline(xd, 1, 512, 48000.0, d.Plugin.conv(taps), out=xd)
    with pytest.raises(d.DspError):
        d.render_offline(xd, 1, 512, 48000.0, d.Plugin.conv(taps), sample_offset=512)
    with pytest.raises(d.DspError):
        d.render_offline(xd, 1, 512, 48000.0, d.Plugin.conv(np.ones((1 << 20) + 1, np.float32)))
    bad = taps.copy()
    bad[17] = np.inf
    with pytest.raises(d.DspError):
        d.render_offline(xd, 1, 512, 48000.0, d.Plugin.conv(bad))
    with pytest.raises(d.DspError):   # FIR did not change
        d.render_offline(xd, 1, 512, 48000.0, d.Plugin.fir(np.ones(2049)))
    torch_cuda.cuda.synchronize()


def test_gpu_conv_long_filter(torch_cuda):
    T, Lx, B = 1 << 18, 300_000, 512
    x, taps = conv_inputs(7, 1, Lx, T)
    y = render(torch_cuda, x, 1, B, taps)[0]
    y64 = conv_f64(x[0], taps, y.size)
    idx = np.unique(np.concatenate([np.arange(64), np.arange(y.size - 64, y.size),
                                    np.random.default_rng(8).integers(0, y.size, 4000)]))
    r = float(np.max(np.abs(y[idx] - y64[idx])) / np.max(np.abs(y64)))
    print(f"conv ratio T=2^18 L={Lx}: {r:.3e}")
    assert r <= CONV_TOL, r
