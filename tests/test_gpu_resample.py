"""dsp_resample on the GPU (csrc/resample.hip) against the definition in
include/dspbench/dspbench.h.

Impulse tests: with x a unit impulse only one product of an output's sum is
nonzero, so every output must equal the dsp_resample_taps entry the definition
names, or 0, bit for bit -- the phase, the indexing and both edges exactly.

Random input (uniform in [-1, 1]) against the float64 model (resampleutil):
per channel max |y - y64| <= RESAMPLE_TOL * max |y64|.  RESAMPLE_TOL is 4 x the
larger of two measured worst ratios over random_cases() below, the rule
test_gpu_conv.py's CONV_TOL follows:
  tools/resample_model.py tol (the same sum in float32 on the CPU):   MODEL32
  the GPU (this file's cases, MI355X):                                GPU32
An indexing mistake is an error of order 1.
"""
import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L
import resampleutil as ru

pytestmark = pytest.mark.gpu

MODEL32 = 1.341e-06
GPU32 = 1.387e-06
RESAMPLE_TOL = 4 * max(MODEL32, GPU32)  # = 5.5e-6

# 160/147, 147/160, 2/1, 1/2, 3/1, 320/147, 1/24
RATES = [(44100, 48000), (48000, 44100), (48000, 96000), (96000, 48000), (16000, 48000), (44100, 96000),
         (48000, 2000)]
ZEROS = (4, 16, 64)


def lengths(sr_in, sr_out, zeros):
    """All-edge calls (1 and Tp - 1 samples), one tile, several tiles with a ragged tail."""
    return (1, ru.plan(sr_in, sr_out, zeros=zeros)["taps"] - 1, 4097, 20000)


def random_cases():
    """Every ratio with every length, every ratio with every zeros, every zeros with every length."""
    out = []
    for i, (a, b) in enumerate(RATES):
        for j in range(4):
            z = ZEROS[(i + j) % 3]
            out.append((a, b, z, lengths(a, b, z)[j]))
    return out


def seed_of(sr_in, sr_out, zeros, Lx):
    return (sr_in * 7 + sr_out * 3 + zeros * 5 + Lx) % (1 << 31)


def ratio(y, y64):
    return float(np.max(np.abs(np.asarray(y, np.float64) - y64)) / max(float(np.max(np.abs(y64))), 1e-30))


def check(y, y64, what):
    r = ratio(y, y64)
    print(f"resample ratio {what}: {r:.3e}")
    assert r <= RESAMPLE_TOL, (what, r)


def run(torch, x, sr_in, sr_out, **kw):
    y = d.resample(torch.from_numpy(np.ascontiguousarray(x)).cuda(), sr_in, sr_out, **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def impulse_want(sr_in, sr_out, zeros, Lx, at):
    """The definition for x = delta[n - at]: y[m] = table[phi][at - (n0 - half + 1)] or 0."""
    p = ru.plan(sr_in, sr_out, Lx, zeros=zeros)
    t = d.resample_taps(sr_in, sr_out, zeros=zeros)
    m = np.arange(p["Lout"], dtype=np.int64)
    q = m * p["down"]
    n0, phi = q // p["up"], q % p["up"]
    i = at - (n0 - p["half"] + 1)
    ok = (i >= 0) & (i < p["taps"])
    return np.where(ok, t[phi, np.clip(i, 0, p["taps"] - 1)], np.float32(0)).astype(np.float32)


@pytest.mark.parametrize("sr_in,sr_out,zeros,Lx", random_cases())
def test_gpu_resample_random(torch_cuda, sr_in, sr_out, zeros, Lx):
    x = ru.inputs(seed_of(sr_in, sr_out, zeros, Lx), 1, Lx)
    y = run(torch_cuda, x, sr_in, sr_out, zeros=zeros)
    assert y.shape == (1, ru.plan(sr_in, sr_out, Lx)["Lout"])
    check(y[0], ru.resample_f64(x[0], sr_in, sr_out, zeros=zeros), f"{sr_in}->{sr_out} Z={zeros} L={Lx}")


@pytest.mark.parametrize("i,rates", list(enumerate(RATES)))
def test_gpu_resample_impulse_is_the_table(torch_cuda, i, rates):
    sr_in, sr_out = rates
    zeros, Lx = ZEROS[i % 3], 20000
    down = ru.plan(sr_in, sr_out)["down"]
    # the first two and the last sample; the first input of the second tile of
    # 64 periods, and of 512 (tiles of few-phase ratios hold up to 1024 periods)
    for at in sorted(n for n in {0, 1, Lx - 1, 64 * down - 1, 64 * down, 512 * down} if n < Lx):
        x = np.zeros((1, Lx), np.float32)
        x[0, at] = 1.0
        y = run(torch_cuda, x, sr_in, sr_out, zeros=zeros)[0]
        want = impulse_want(sr_in, sr_out, zeros, Lx, at)
        assert y.shape == want.shape
        assert np.array_equal(y, want), (sr_in, sr_out, zeros, at, int(np.argmax(y != want)))


def test_gpu_resample_impulse_short_input(torch_cuda):
    """L = 1: the whole call is edge; y is one column of the table."""
    for sr_in, sr_out in RATES:
        y = run(torch_cuda, np.ones((1, 1), np.float32), sr_in, sr_out, zeros=4)[0]
        assert np.array_equal(y, impulse_want(sr_in, sr_out, 4, 1, 0)), (sr_in, sr_out)


@pytest.mark.parametrize("sr_in,sr_out,zeros,Lx", [(11025, 192000, 4, 4097), (192000, 11025, 4, 20000),
                                                   (192000, 11025, 16, 4097)])
def test_gpu_resample_large_ratio_terms(torch_cuda, sr_in, sr_out, zeros, Lx):
    """up = 2560 / down = 2560: a tile of 64 periods does not fit in LDS, the
    one-output-per-lane kernel runs.  Same checks."""
    x = ru.inputs(seed_of(sr_in, sr_out, zeros, Lx), 1, Lx)
    y = run(torch_cuda, x, sr_in, sr_out, zeros=zeros)
    check(y[0], ru.resample_f64(x[0], sr_in, sr_out, zeros=zeros), f"{sr_in}->{sr_out} Z={zeros} L={Lx}")
    for at in (0, 1, Lx - 1, Lx // 2):
        xi = np.zeros((1, Lx), np.float32)
        xi[0, at] = 1.0
        assert np.array_equal(run(torch_cuda, xi, sr_in, sr_out, zeros=zeros)[0],
                              impulse_want(sr_in, sr_out, zeros, Lx, at)), at


def test_gpu_resample_same_rate_is_a_copy(torch_cuda):
    x = ru.inputs(3, 2, 4097)
    x[0, 5] = np.float32("nan")   # a copy keeps every bit pattern
    y = run(torch_cuda, x, 48000, 48000)
    assert y.shape == x.shape and np.array_equal(y.view(np.uint32), x.view(np.uint32))


@pytest.fixture(scope="module")
def chan_ref():
    x = ru.inputs(11, 17, 4097)
    return x, [ru.resample_f64(x[c], 44100, 48000, zeros=16) for c in range(17)]


@pytest.mark.parametrize("C", [1, 2, 17])
def test_gpu_resample_channels(torch_cuda, chan_ref, C):
    x, ref = chan_ref
    y = run(torch_cuda, x[:C], 44100, 48000, zeros=16)
    assert y.shape == (C, ref[0].size)
    for c in range(C):
        check(y[c], ref[c], f"C={C} c={c}")


def test_gpu_resample_host_buffers_and_stream(torch_cuda, chan_ref):
    x, ref = chan_ref
    dev = run(torch_cuda, x[:2], 44100, 48000, zeros=16)
    host = d.resample(x[:2], 44100, 48000, zeros=16)          # numpy in, numpy out: DSP_EXEC_HOST_BUFFERS
    assert isinstance(host, np.ndarray) and np.array_equal(host, dev)
    s = torch_cuda.cuda.Stream()
    xd = torch_cuda.from_numpy(x[:2]).cuda()
    torch_cuda.cuda.synchronize()
    y = d.resample(xd, 44100, 48000, zeros=16, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(y.cpu().numpy(), dev)
    check(dev[1], ref[1], "host / stream")


def test_gpu_resample_defaults_are_kaiser_best(torch_cuda):
    x = ru.inputs(5, 1, 4097)
    a = run(torch_cuda, x, 44100, 48000)
    b = run(torch_cuda, x, 44100, 48000, zeros=64, beta=14.769656459379492, rolloff=0.9475937167399596)
    assert np.array_equal(a, b)
    c = run(torch_cuda, x, 44100, 48000, beta=8.0)   # another table under another cache key
    assert not np.array_equal(a, c)
    check(c[0], ru.resample_f64(x[0], 44100, 48000, beta=8.0), "beta 8")


def test_gpu_resample_refusals(torch_cuda):
    x = torch_cuda.from_numpy(ru.inputs(6, 1, 4097)).cuda()
    lib = L.lib()
    ex = L.dsp_exec(-1, L.DSP_EXEC_SYNC, None, 0)
    rows = L.chan_table([x.data_ptr()])
    out = torch_cuda.empty((1, 4460), device="cuda")
    orow = L.chan_table([out.data_ptr()])
    import ctypes as C
    assert d.resample_plan(44100, 48000, 4097)["Lout"] == 4460
    assert lib.dsp_resample(rows, 1, 4097, orow, 4460, 44100, 48000, None, C.byref(ex)) == L.DSP_OK
    assert lib.dsp_resample(rows, 1, 4097, orow, 4459, 44100, 48000, None, C.byref(ex)) == L.DSP_ERR_INVALID  # Lout
    assert lib.dsp_resample(rows, 1, 4097, rows, 4460, 44100, 48000, None, C.byref(ex)) == L.DSP_ERR_INVALID  # in place
    assert lib.dsp_resample(rows, 1, 4097, orow, 4460, 44100, 0, None, C.byref(ex)) == L.DSP_ERR_INVALID
    exo = L.dsp_exec(-1, L.DSP_EXEC_SYNC, None, 512)
    assert lib.dsp_resample(rows, 1, 4097, orow, 4460, 44100, 48000, None, C.byref(exo)) == L.DSP_ERR_INVALID
    assert lib.dsp_resample(rows, 1, 4097, orow, 4460, 4099, 4097, None, C.byref(ex)) == L.DSP_ERR_UNSUPPORTED
    assert lib.dsp_resample(rows, 1, 0, orow, 0, 44100, 48000, None, C.byref(ex)) == L.DSP_OK   # L = 0: nothing
    torch_cuda.cuda.synchronize()
