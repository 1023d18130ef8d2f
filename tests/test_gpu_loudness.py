"""dsp_loudness on the GPU (csrc/loudness.hip) against the float64 model
(loudnessutil) of the definition in include/dspbench/dspbench.h.

Hop energy: per channel max_j |z - z64| <= LOUD_TOL * max_j z64.  LOUD_TOL is
4 x the larger of two measured worst ratios over hop_cases(), channel_cases()
and long_cases() below, the rule CONV_TOL and RESAMPLE_TOL follow:
  tools/loudness_model.py tol (oracle.biquad_f32, the squares summed in
  float64):                                                       MODEL32 = 1.869e-5
  the GPU (this file's cases, MI355X):                            GPU32 = 1.467e-4
Both worst cases are the 192 kHz second-run case (48 kHz: 2.2e-6 and 4.2e-6;
192 kHz inside the first run: 1.1e-5 and 1.4e-4).
A dropped or misplaced tile state is an error above 1e-2.

Integrated loudness: |integrated - model| <= (10 / ln 10) LOUD_TOL max z /
(mean gated z), computed from the model, on inputs whose model block loudness
stays >= 0.01 LU from both gates.

True peak: an impulse gives a table entry times the amplitude bit for bit;
random input is within test_gpu_resample's RESAMPLE_TOL of the float64 model's
peak (max is 1-Lipschitz).
"""
import ctypes as C
import gc

import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L
import loudnessutil as lu
import resampleutil as ru
from test_gpu_resample import RESAMPLE_TOL

pytestmark = pytest.mark.gpu

MODEL32 = 1.869e-05
GPU32 = 1.467e-04
LOUD_TOL = 4 * max(MODEL32, GPU32)  # = 5.9e-4

RATES = (8000, 44100, 48000, 192000)
FIELDS = ("integrated", "range", "momentary_max", "short_term_max", "blocks", "gated_blocks")


def lengths(sr):
    hop = lu.plan(sr)["hop"]
    return (1, hop - 1, 4 * hop - 1, 4 * hop, 2047, 2048, 2049, 20000, 100003, 14 * 2048 + 5)


def hop_cases():
    """Every rate with every length, one channel."""
    return [(sr, Lx) for sr in RATES for Lx in lengths(sr)]


def channel_cases():
    """Every channel count (a single, a pair, a pair and a single, two groups) with two lengths."""
    return [(Cn, Lx) for Cn in (1, 2, 3, 17) for Lx in (20000, 14 * 2048 + 5)]


CHANNEL_RATE = 48000


def run_tiles(sr):
    """(W, R): a wave measures a run of R = max(32, 8 W) tiles of 2048 samples after a warm-up of W tiles
    from a zero state, W = dsp_biquad_plan's look-back window of the rate's cascade."""
    w = C.c_uint32()
    k = d.k_weighting(sr)
    fn = L.lib().dsp_biquad_plan
    fn.argtypes, fn.restype = [L.FP, C.c_uint32, C.POINTER(C.c_uint32)], C.c_int
    assert fn(k.ctypes.data_as(L.FP), 2, C.byref(w)) == L.DSP_OK and w.value >= 1
    return w.value, max(32, 8 * w.value)


def long_cases():
    """(sr, channels, L): past the first run and the second's warm-up at the rates whose run is longer than
    every length above (96 kHz: 72 tiles, 192 kHz: 144), so that hops of a run entered from a warm-up are
    checked; one channel and a pair."""
    return [(96000, 1, 180003), (96000, 2, 180003), (192000, 1, 365003), (192000, 2, 365003)]


def seed_of(sr, Lx):
    return (sr * 7 + Lx * 3) % (1 << 31)


def ratio(z, z64):
    return float(np.max(np.abs(z - z64)) / max(float(np.max(z64)), 1e-300)) if z64.size else 0.0


def measure(torch, x, sr, **kw):
    r = d.loudness(torch.from_numpy(np.ascontiguousarray(x)).cuda(), sr, **kw)
    torch.cuda.synchronize()
    return r


def same_as_own_gate(r, hop, weights=None):
    g = d.loudness_gate(r["hop_energy"], hop, weights)
    for k in FIELDS:
        assert r[k] == g[k], (k, r[k], g[k])


@pytest.mark.parametrize("sr,Lx", hop_cases())
def test_gpu_loudness_hop_energy(torch_cuda, oracle, sr, Lx):
    x = lu.noise(seed_of(sr, Lx), 1, Lx)
    r = measure(torch_cuda, x, sr, true_peak=False)
    p = lu.plan(sr, Lx)
    assert r["hop_energy"].shape == (1, p["hops"])
    z64 = lu.hop_energy64(x[0], sr)
    q = ratio(r["hop_energy"][0], z64)
    print(f"loudness ratio sr={sr} L={Lx}: {q:.3e}")
    assert q <= LOUD_TOL, (sr, Lx, q)
    assert r["sample_peak"] == float(np.max(np.abs(x))) and r["channel_peaks"][0, 0] == r["sample_peak"]
    assert np.isnan(r["true_peak"]) and np.isnan(r["channel_peaks"][0, 1])
    assert r["blocks"] == max(p["hops"] - 3, 0)
    same_as_own_gate(r, p["hop"])
    if p["hops"] < 4:
        assert r["integrated"] == -np.inf and r["momentary_max"] == -np.inf


@pytest.fixture(scope="module")
def chan_ref(oracle):
    Lmax = 14 * 2048 + 5
    x = lu.noise(77, 17, Lmax)
    return x, {Lx: [lu.hop_energy64(x[c, :Lx], CHANNEL_RATE) for c in range(17)] for Lx in (20000, Lmax)}


@pytest.mark.parametrize("Cn,Lx", channel_cases())
def test_gpu_loudness_channels(torch_cuda, chan_ref, Cn, Lx):
    x, ref = chan_ref
    r = measure(torch_cuda, x[:Cn, :Lx], CHANNEL_RATE, true_peak=False)
    assert r["hop_energy"].shape == (Cn, Lx // 4800)
    for c in range(Cn):
        q = ratio(r["hop_energy"][c], ref[Lx][c])
        print(f"loudness ratio C={Cn} c={c} L={Lx}: {q:.3e}")
        assert q <= LOUD_TOL, (Cn, c, Lx, q)
        assert r["channel_peaks"][c, 0] == float(np.max(np.abs(x[c, :Lx])))
    assert r["sample_peak"] == float(np.max(np.abs(x[:Cn, :Lx])))
    same_as_own_gate(r, 4800)


@pytest.mark.parametrize("sr,Cn,Lx", long_cases())
def test_gpu_loudness_second_run(torch_cuda, oracle, sr, Cn, Lx):
    W, R = run_tiles(sr)
    p = lu.plan(sr, Lx)
    first = -(-R * 2048 // p["hop"])                 # the first hop wholly inside the second run
    assert Lx > (R + W) * 2048 and p["hops"] - first >= 2, (W, R)
    assert max(lengths(sr)) <= R * 2048              # (why the cases above never leave the first run here)
    x = lu.noise(seed_of(sr, Lx) + 5, Cn, Lx)
    r = measure(torch_cuda, x, sr, true_peak=False)
    for c in range(Cn):
        z64 = lu.hop_energy64(x[c], sr)
        q = ratio(r["hop_energy"][c], z64)
        q2 = float(np.max(np.abs(r["hop_energy"][c][first:] - z64[first:])) / np.max(z64))
        print(f"loudness ratio long sr={sr} C={Cn} c={c} L={Lx}: {q:.3e} (second run {q2:.3e})")
        assert q <= LOUD_TOL, (sr, Cn, c, q)
    same_as_own_gate(r, p["hop"])


def result_input(sr, kind):
    Lx = 20000 if sr == 8000 else 100003
    x = lu.noise(seed_of(sr, Lx) + 1, 2, Lx, 0.5)
    if kind == "step":      # the second half 15 LU down: the relative gate removes it
        x[:, Lx // 2:] *= np.float32(10.0 ** (-15.0 / 20.0))
    return x


@pytest.mark.parametrize("sr", RATES)
@pytest.mark.parametrize("kind", ["noise", "step"])
def test_gpu_loudness_integrated(torch_cuda, oracle, sr, kind):
    x = result_input(sr, kind)
    m = lu.loudness64(x, sr)
    assert m["blocks"] >= 1 and m["margin"] >= 0.01, m["margin"]
    r = measure(torch_cuda, x, sr, true_peak=False)
    same_as_own_gate(r, lu.plan(sr)["hop"])
    assert (r["blocks"], r["gated_blocks"]) == (m["blocks"], m["gated_blocks"])
    if kind == "step" and m["blocks"] > 4:
        assert m["gated_blocks"] < m["blocks"]
    # a gated block's power moves by at most LOUD_TOL max z per hop of its four, per channel
    zmax = sum(float(np.max(m["hop_energy"][c])) for c in range(2))
    bound = (10.0 / np.log(10.0)) * LOUD_TOL * zmax / (m["gated_mean"] * lu.plan(sr)["hop"])
    err = abs(r["integrated"] - m["integrated"])
    print(f"loudness integrated sr={sr} {kind}: {r['integrated']:.6f} model {m['integrated']:.6f} "
          f"err {err:.3e} bound {bound:.3e}")
    assert err <= bound


def test_gpu_loudness_weights(torch_cuda, oracle):
    x = lu.noise(9, 3, 30000, 0.5)
    w = [1.0, 0.0, 1.41]
    r = measure(torch_cuda, x, 48000, weights=w, true_peak=False)
    same_as_own_gate(r, 4800, w)
    plain = measure(torch_cuda, x, 48000, true_peak=False)
    assert np.array_equal(r["hop_energy"], plain["hop_energy"]) and r["integrated"] != plain["integrated"]


def test_gpu_loudness_is_reproducible(torch_cuda):
    x = lu.noise(3, 3, 100003)
    a = measure(torch_cuda, x, 44100)
    b = measure(torch_cuda, x, 44100)
    assert np.array_equal(a["hop_energy"].view(np.uint64), b["hop_energy"].view(np.uint64))
    assert a["true_peak"] == b["true_peak"] and a["integrated"] == b["integrated"]
    # a channel's energies do not depend on the channels beside it (a pair, or alone)
    alone = measure(torch_cuda, x[1:2], 44100, true_peak=False)
    assert np.array_equal(alone["hop_energy"][0].view(np.uint64), a["hop_energy"][1].view(np.uint64))


@pytest.mark.parametrize("at", ["first", "last", "tile_end", "tile_start"])
def test_gpu_loudness_sample_peak_is_exact(torch_cuda, at):
    Lx = 2 * 4800 + 2048 + 77          # the last sample sits in the ragged tail past the last hop
    n = {"first": 0, "last": Lx - 1, "tile_end": 2047, "tile_start": 4096}[at]
    x = lu.noise(21, 2, Lx, 0.5)
    x[1, n] = np.float32(-0.875)
    r = measure(torch_cuda, x, 48000, true_peak=False)
    assert r["sample_peak"] == 0.875
    assert r["channel_peaks"][1, 0] == 0.875 and r["channel_peaks"][0, 0] == float(np.max(np.abs(x[0])))


def test_gpu_loudness_ebu_sine(torch_cuda):
    """EBU Tech 3341 case 1: a stereo 1 kHz sine at -23 dBFS measures -23.0 +- 0.1 LUFS."""
    r = measure(torch_cuda, lu.sine(48000, 5, 1000.0, -23.0, 2), 48000)
    assert abs(r["integrated"] - -23.0) <= 0.1, r["integrated"]
    assert r["blocks"] == 47 and r["gated_blocks"] == 47


def impulse_peak(sr, ovs, zeros, Lx, at, amp):
    """max |amp t| over the table entries the definition reaches inside [0, L)."""
    p = ru.plan(sr, ovs * sr, Lx, zeros=zeros)
    t = d.resample_taps(sr, ovs * sr, zeros=zeros)
    i = at - np.arange(Lx, dtype=np.int64) + p["half"] - 1      # the tap that meets x[at] for each n0
    i = i[(i >= 0) & (i < p["taps"])]
    return float(np.max(np.abs(np.float32(amp) * t[:, i])))


@pytest.mark.parametrize("sr,ovs", [(48000, 4), (96000, 2)])
@pytest.mark.parametrize("zeros", [4, 64])
def test_gpu_loudness_true_peak_impulse_is_the_table(torch_cuda, sr, ovs, zeros):
    Lx, amp = 4097, np.float32(0.7)
    assert lu.plan(sr)["oversample"] == ovs
    for at in (0, 1, Lx - 1, 1023, 1024):      # both edges; the last input of a staging tile, the next one's first
        x = np.zeros((1, Lx), np.float32)
        x[0, at] = amp
        r = measure(torch_cuda, x, sr, zeros=zeros)
        assert r["true_peak"] == impulse_peak(sr, ovs, zeros, Lx, at, amp), (sr, zeros, at)
        assert r["sample_peak"] == float(amp)


@pytest.mark.parametrize("Lx", [1, 4097, 20000])
def test_gpu_loudness_true_peak_random(torch_cuda, Lx):
    x = lu.noise(40 + Lx, 2, Lx)
    r = measure(torch_cuda, x, 48000)
    for c in range(2):
        y64 = ru.resample_f64(x[c], 48000, 192000)
        want = float(np.max(np.abs(y64)))
        assert abs(r["channel_peaks"][c, 1] - want) <= RESAMPLE_TOL * want, (c, r["channel_peaks"][c, 1], want)
    assert r["true_peak"] == r["channel_peaks"][:, 1].max()


def test_gpu_loudness_true_peak_at_192k_is_the_sample_peak(torch_cuda):
    x = lu.noise(50, 2, 20000)
    r = measure(torch_cuda, x, 192000)
    assert r["true_peak"] == r["sample_peak"] == float(np.max(np.abs(x)))
    assert np.array_equal(r["channel_peaks"][:, 0], r["channel_peaks"][:, 1])


def test_gpu_loudness_true_peak_between_samples(torch_cuda):
    """A sine at sr / 4 with 45 degrees of phase: every sample is +-0.7071, the peak between them is 1."""
    x = lu.sine(48000, 0.25, 12000.0, 0.0, 1, phase=np.pi / 4)
    r = measure(torch_cuda, x, 48000)
    assert abs(r["sample_peak"] - np.sqrt(0.5)) < 1e-6
    want = float(np.max(np.abs(ru.resample_f64(x[0], 48000, 192000))))
    assert abs(want - 1.0) < 0.05          # (the model's own: 1.0117, the sine starts abruptly)
    assert abs(r["true_peak"] - want) <= RESAMPLE_TOL * want


def test_gpu_loudness_host_rows_and_stream(torch_cuda):
    x = lu.noise(60, 3, 30011)
    dev = measure(torch_cuda, x, 44100)
    host = d.loudness(x, 44100)                       # numpy in: DSP_EXEC_HOST_BUFFERS
    s = torch_cuda.cuda.Stream()
    xd = torch_cuda.from_numpy(x).cuda()
    torch_cuda.cuda.synchronize()
    side = d.loudness(xd, 44100, stream=s.cuda_stream)
    for other in (host, side):
        assert np.array_equal(other["hop_energy"].view(np.uint64), dev["hop_energy"].view(np.uint64))
        assert np.array_equal(other["channel_peaks"], dev["channel_peaks"])
        for k in FIELDS + ("sample_peak", "true_peak"):
            assert other[k] == dev[k], k


def test_gpu_loudness_refuses_a_capturing_stream(torch_cuda):
    torch = torch_cuda
    x = torch.from_numpy(lu.noise(61, 1, 20000)).cuda()
    d.loudness(x, 48000)                              # an eager call first: tables and scratch exist
    torch.cuda.synchronize()
    gc.collect()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    msg = None
    try:
        with torch.cuda.graph(g, stream=side):
            d.loudness(x, 48000)
    except Exception as e:  # noqa: BLE001
        msg = str(e)
    torch.cuda.synchronize()
    del g
    gc.collect()
    assert msg is not None and "capture" in msg, msg


def test_gpu_loudness_argument_errors(torch_cuda):
    x = torch_cuda.from_numpy(lu.noise(62, 1, 20000)).cuda()
    lib = L.lib()
    rows = L.chan_table([x.data_ptr()])
    res = L.dsp_loudness_result()
    ex = L.dsp_exec(-1, L.DSP_EXEC_SYNC, None, 0)

    def call(rows_=rows, C_=1, L_=20000, sr=48000, res_=C.byref(res), ex_=ex, flags=0):
        return lib.dsp_loudness(rows_, C_, L_, sr, None, flags, None, None, None, res_, C.byref(ex_))

    assert call() == L.DSP_OK and res.blocks == 1
    assert call(C_=0) == L.DSP_ERR_INVALID
    assert call(rows_=L.chan_table([0])) == L.DSP_ERR_INVALID
    assert call(res_=None) == L.DSP_ERR_INVALID
    assert call(sr=7999) == L.DSP_ERR_UNSUPPORTED and call(sr=384001) == L.DSP_ERR_UNSUPPORTED
    assert call(ex_=L.dsp_exec(-1, L.DSP_EXEC_SYNC, None, 512)) == L.DSP_ERR_INVALID
    assert call(flags=2) == L.DSP_ERR_INVALID
    assert call(L_=0) == L.DSP_OK                     # nothing to measure: -inf, no peaks
    assert res.integrated == -np.inf and res.blocks == 0 and res.sample_peak == 0.0 and np.isnan(res.true_peak)
    assert call(L_=0, flags=1) == L.DSP_OK and res.true_peak == 0.0
    torch_cuda.cuda.synchronize()
