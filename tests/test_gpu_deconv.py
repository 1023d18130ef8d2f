"""dsp_rfft / dsp_irfft / dsp_deconvolve on the GPU (fft_big.hip) against the
float64 models of tests/deconvutil.py and against themselves: closed forms at
the pass seams, spectra, zero padding, row layouts, channel groups,
reproducibility, the deconvolution cases, refusals and modes.  Device results
and float64 references are computed once per (n) or case and shared."""
import ctypes
import functools

import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L
import deconvutil as du
import rowsutil as ru

pytestmark = pytest.mark.gpu

NS = du.FFT_NS


def cplx(spec):
    """[C, n + 2] float32 -> [C, n / 2 + 1] complex128."""
    s = np.asarray(spec, np.float64)
    return s[:, 0::2] + 1j * s[:, 1::2]


def gpu_rfft(torch, x, n, L_=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return d.rfft(t, n, L_).cpu().numpy()


def e_fft(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def test_plans_cover_every_instantiation():
    """The n of this file run every pass count (2, 3, 4) and every radix (64, 32, 8) the kernels are built for."""
    plans = [d.rfft_plan(n) for n in NS + (du.BIG_N,)]
    assert {p["passes"] for p in plans} == {2, 3, 4}
    assert {r for p in plans for r in p["radix"]} == {64, 32, 8}
    every = [d.rfft_plan(1 << b) for b in range(10, 25)]
    assert {p["passes"] for p in every} == {2, 3, 4} and {r for p in every for r in p["radix"]} == {64, 32, 8}
    # a first pass and a later pass of every radix
    assert {p["radix"][0] for p in plans} == {64, 32} == {p["radix"][0] for p in every}
    assert {r for p in plans for r in p["radix"][1:]} == {64, 32, 8}


@functools.lru_cache(None)
def seam_run(n):
    """Every closed-form row of n in one call: (names, spectra [rows, n / 2 + 1] complex128)."""
    import torch
    rows, names = [], []
    for j in du.impulse_positions(n):
        x = np.zeros(n, np.float32)
        x[j] = 1.0
        rows.append(x)
        names.append(("impulse", j))
    for k in du.cosine_bins(n):
        rows.append(du.cosine(n, k))
        names.append(("cos", k))
    return names, cplx(gpu_rfft(torch, np.stack(rows), n))


@pytest.mark.parametrize("n", NS)
def test_seams_closed_forms(torch_cuda, n):
    names, X = seam_run(n)
    k = np.arange(n // 2 + 1)
    for (kind, v), got in zip(names, X):
        if kind == "impulse":
            want = np.exp(-2j * np.pi * v * k / n)
        else:
            # the float32 cosine's own spectrum: n / 2 at bin v (n at 0 and n / 2), and its rounding noise
            want = du.rfft64(du.cosine(n, v), n)
            ideal = np.zeros(n // 2 + 1)
            ideal[v] = n if v in (0, n // 2) else n / 2
            assert np.max(np.abs(want - ideal)) <= 1e-6 * n
        err = e_fft(got, want)
        assert err <= du.FFT_TOL, (kind, v, err)


@functools.lru_cache(None)
def spectrum_run(n):
    import torch
    x = np.zeros((2, n), np.float32)
    x[0] = du.noise(n, 1, n)[0]
    x[1, :n - 3] = du.decay(n - 3)
    spec = gpu_rfft(torch, x, n)
    back = d.irfft(torch.from_numpy(spec).cuda(), n).cpu().numpy()
    x.setflags(write=False)
    return x, spec, back


@pytest.mark.parametrize("n", NS)
def test_spectrum_and_round_trip(torch_cuda, n):
    x, spec, back = spectrum_run(n)
    X = cplx(spec)
    for c in range(2):
        err = e_fft(X[c], du.rfft64(x[c], n))
        print(f"n={n} row {c}: e_fft = {err:.3e}")
        assert err <= du.FFT_TOL
        # the inverse of the device's own spectrum, against float64's inverse of it; and the round trip
        want = np.fft.irfft(X[c], n)
        assert np.max(np.abs(back[c] - want)) <= du.FFT_TOL * np.max(np.abs(want))
        assert np.max(np.abs(back[c] - x[c])) <= 2 * du.FFT_TOL * np.max(np.abs(x[c]))


def test_big_transform(torch_cuda):
    """n = 2^24, C = 1: four passes; an impulse at the last radix's seam, then noise, then back."""
    n = du.BIG_N
    r = d.rfft_plan(n)["radix"][-1]
    x = np.zeros((1, n), np.float32)
    x[0, r + 1] = 1.0
    k = np.arange(n // 2 + 1)
    X = cplx(gpu_rfft(torch_cuda, x, n))[0]
    assert e_fft(X, np.exp(-2j * np.pi * ((r + 1) * k % n) / n)) <= du.FFT_TOL
    x = du.noise(n, 1, n)
    t = torch_cuda.from_numpy(x).cuda()
    spec = d.rfft(t, n)
    err = e_fft(cplx(spec.cpu().numpy())[0], du.rfft64(x[0], n))
    print(f"n=2^24 noise: e_fft = {err:.3e}")
    assert err <= du.FFT_TOL
    back = d.irfft(spec, n).cpu().numpy()
    assert np.max(np.abs(back - x)) <= 2 * du.FFT_TOL


@pytest.mark.parametrize("n", [1 << 10, 1 << 14])
def test_zero_padding_and_lout(torch_cuda, n):
    x = du.noise(n + 1, 1, n)
    for L_ in (0, 1, n // 2 - 1, n // 2 + 1, n - 1, n):
        # L_ samples, NaN behind them: the frame's zeros are never read from memory
        rows = ru.Rows(1, n, 0, 0, torch_cuda).fill(x, L_)
        spec = d.rfft(rows.view, n, L_).cpu().numpy()
        ru.assert_finite(spec)
        want = du.rfft64(x[0, :L_], n)
        if L_ == 0:
            assert not spec.any()
        else:
            assert e_fft(cplx(spec)[0], want) <= du.FFT_TOL
    spec = torch_cuda.from_numpy(gpu_rfft(torch_cuda, x, n)).cuda()
    whole = d.irfft(spec, n).cpu().numpy()
    for Lout in (1, n // 2 - 1, n // 2 + 1, n - 1):
        out = ru.Rows(1, n, 0, 0, torch_cuda)
        d.irfft(spec, n, Lout, out=out.view)
        out.check_output(Lout)  # nothing past Lout
        assert ru.same_bits(out.numpy(Lout), whole[:, :Lout])


@functools.lru_cache(None)
def channels_base(n, C):
    import torch
    x = du.noise(7 * n + C, C, n - 5)
    spec = d.rfft(torch.from_numpy(x).cuda(), n)
    back = d.irfft(spec, n, n - 5)
    return x, spec.cpu().numpy(), back.cpu().numpy()


@pytest.mark.parametrize("C", [1, 2, 3, 16, 17])
def test_channels_bitwise(torch_cuda, C):
    """Across the channel-group boundary: channel c is the C = 1 call's bits, and two runs agree."""
    n = 1 << 12
    x, spec, back = channels_base(n, C)
    x2, spec2, back2 = channels_base.__wrapped__(n, C)
    assert ru.same_bits(spec, spec2) and ru.same_bits(back, back2)
    for c in sorted({0, C - 1, C // 2}):
        t = torch_cuda.from_numpy(x[c:c + 1]).cuda()
        s1 = d.rfft(t, n)
        assert ru.same_bits(s1.cpu().numpy(), spec[c:c + 1])
        assert ru.same_bits(d.irfft(s1, n, n - 5).cpu().numpy(), back[c:c + 1])


@pytest.mark.parametrize("layout", ru.ALL)
def test_rows_fft(torch_cuda, layout):
    """Unaligned starts, strided rows, NaN guards: rfft and irfft write only their rows and give the aligned call's bits."""
    n, C, Lx = 1 << 11, 3, (1 << 11) - 7
    x, spec0, back0 = rows_base(n, C, Lx)
    oi, oo, sm = ru.LAYOUTS[layout]
    for host in (False, True):
        t = None if host else torch_cuda
        xin = ru.Rows(C, Lx + 5, oi, sm, t).fill(x, Lx)
        spec = ru.Rows(C, n + 2, oo, sm, t)
        ex = d.api._exec(xin.view if not host else None, 0, None, sync=True)
        L.check(L.lib().dsp_rfft(L.chan_table(xin.ptrs()), C, Lx, n, L.chan_table(spec.ptrs()), ctypes.byref(ex)),
                "dsp_rfft")
        spec.check_output()
        assert ru.same_bits(spec.numpy(), spec0)
        sin = ru.Rows(C, n + 2, oi, sm, t).fill(spec0)
        out = ru.Rows(C, Lx, oo, sm, t)
        L.check(L.lib().dsp_irfft(L.chan_table(sin.ptrs()), C, n, L.chan_table(out.ptrs()), Lx, ctypes.byref(ex)),
                "dsp_irfft")
        out.check_output()
        assert ru.same_bits(out.numpy(), back0)


@functools.lru_cache(None)
def rows_base(n, C, Lx):
    import torch
    x = du.noise(n + C + Lx, C, Lx)
    spec = d.rfft(torch.from_numpy(x).cuda(), n)
    return x, spec.cpu().numpy(), d.irfft(spec, n, Lx).cpu().numpy()


# ---------------------------------------------------------------------------
# deconvolution
# ---------------------------------------------------------------------------
DEC_IDS = [k["name"] for k in du.DEC_CASES]


def gpu_deconv(torch, rec, ref, **kw):
    return d.deconvolve(torch.from_numpy(np.ascontiguousarray(rec)).cuda(), torch.from_numpy(np.ascontiguousarray(ref)).cuda(),
                        **kw).cpu().numpy()


@functools.lru_cache(None)
def dec_run(i):
    import torch
    k = du.DEC_CASES[i]
    rec, ref = du.dec_case_input(k)
    got = gpu_deconv(torch, rec, ref, ir_len=k["ir_len"], eps=k["eps"], pre=k["pre"])
    want = du.deconv64(rec, ref, k["eps"], k["pre"], k["ir_len"])
    return rec, ref, got, want


@pytest.mark.parametrize("i", range(len(du.DEC_CASES)), ids=DEC_IDS)
def test_deconvolve_model(torch_cuda, i):
    k = du.DEC_CASES[i]
    rec, ref, got, want = dec_run(i)
    assert got.shape == want.shape
    ru.assert_finite(got)
    # (a window of one or a few samples may hold no energy: the whole response's peak is the scale)
    scale = np.max(np.abs(du.deconv64(rec, ref, k["eps"], 0, None)))
    err = float(np.max(np.abs(got - want)) / scale)
    print(f"{k['name']}: e_dec = {err:.3e}")
    assert err <= du.DEC_TOL


def test_deconvolve_recovers_the_known_response(torch_cuda):
    """The float64 model recovers the band-limited h within RECOVERY_TOL (the method); the GPU is within DEC_TOL of the model."""
    i = DEC_IDS.index("sweep-eps6")
    rec, ref, got, want = dec_run(i)
    h = np.zeros(want.shape[1])
    h[:1024] = du.bandpass_ir(L=1024)
    rel = np.max(np.abs(want[0] - h)) / np.max(np.abs(h))
    print(f"recovery (float64 model): {rel:.3e}")
    assert rel <= du.RECOVERY_TOL
    assert np.max(np.abs(got[0] - h)) / np.max(np.abs(h)) <= du.RECOVERY_TOL + du.DEC_TOL
    assert int(np.argmax(np.abs(got[1]))) == int(np.argmax(np.abs(h))) + 5  # row 1: 0.5 h, 5 samples late


@pytest.mark.parametrize("pre", [0, 1, 777])
def test_deconvolve_identity(torch_cuda, pre):
    """rec = ref: a unit impulse at index pre (1 / (1 + eps) where the excitation has energy)."""
    ref = du.noise(3, 1, 3000)[0]
    got = gpu_deconv(torch_cuda, ref[None, :], ref, ir_len=1024, eps=1e-6, pre=pre)[0]
    want = du.deconv64(ref[None, :], ref, 1e-6, pre, 1024)[0]
    assert int(np.argmax(np.abs(got))) == pre and abs(got[pre] - 1.0) <= 1e-2
    assert np.max(np.abs(got - want)) <= du.DEC_TOL


def test_deconvolve_harmonics(torch_cuda):
    """x + 0.1 x^2 + 0.05 x^3 of the sweep: orders 2 and 3 peak where dsp_sweep_harmonic_offset says, +- 2 samples."""
    s = du.SWEEP
    ref = d.sweep(s["sr"], s["f1"], s["f2"], s["seconds"], s["amplitude"], s["fade"])
    x = ref.astype(np.float64)
    rec = (x + 0.1 * x ** 2 + 0.05 * x ** 3).astype(np.float32)[None, :]
    n = d.deconv_plan(rec.shape[1], ref.size)["n"]
    h = gpu_deconv(torch_cuda, rec, ref, ir_len=n, eps=1e-6, pre=n // 2)[0]
    assert int(np.argmax(np.abs(h))) == n // 2
    for order in (2, 3):
        off = d.sweep_harmonic_offset(s["sr"], s["f1"], s["f2"], s["seconds"], order)
        at = n // 2 - int(round(off))
        w = 200  # a window that holds this order's response and no other
        peak = at - w + int(np.argmax(np.abs(h[at - w:at + w])))
        assert abs(peak - at) <= 2, (order, peak, at)


@pytest.mark.parametrize("layout", ru.FEW)
def test_rows_deconvolve(torch_cuda, layout):
    C, Ly, Ls, irl, pre = 3, 1500, 1100, 1301, 3
    rec, ref = du.noise(1, C, Ly), du.noise(2, 1, Ls)
    base = gpu_deconv(torch_cuda, rec, ref[0], ir_len=irl, eps=1e-6, pre=pre)
    oi, oo, sm = ru.LAYOUTS[layout]
    sp = L.dsp_deconv_spec(1e-6, pre)
    for host in (False, True):
        t = None if host else torch_cuda
        rin = ru.Rows(C, Ly + 5, oi, sm, t).fill(rec, Ly)
        fin = ru.Rows(1, Ls + 3, oi if isinstance(oi, int) else 1, 0, t).fill(ref, Ls)
        out = ru.Rows(C, irl, oo, sm, t)
        ex = d.api._exec(rin.view if not host else None, 0, None)
        L.check(L.lib().dsp_deconvolve(L.chan_table(rin.ptrs()), C, Ly, ctypes.cast(ctypes.c_void_p(fin.ptrs()[0]), L.FP),
                                       Ls, L.chan_table(out.ptrs()), irl, ctypes.byref(sp), ctypes.byref(ex)),
                "dsp_deconvolve")
        if not host:
            torch_cuda.cuda.synchronize()
        out.check_output()
        got = out.numpy()
        ru.assert_finite(got)
        assert ru.same_bits(got, base)  # host rows equal device rows bit for bit


@pytest.mark.parametrize("C", [2, 17])
def test_deconvolve_channels_bitwise(torch_cuda, C):
    rec, ref = du.noise(C, C, 2000), du.noise(99, 1, 2048)[0]
    a = gpu_deconv(torch_cuda, rec, ref, ir_len=512, pre=7)
    b = gpu_deconv(torch_cuda, rec, ref, ir_len=512, pre=7)
    assert ru.same_bits(a, b)
    for c in (0, C - 1):
        assert ru.same_bits(gpu_deconv(torch_cuda, rec[c:c + 1], ref, ir_len=512, pre=7), a[c:c + 1])


def test_deconvolve_refusals(torch_cuda):
    rec = torch_cuda.zeros((2, 2048), dtype=torch_cuda.float32, device="cuda") + 0.25
    zero = torch_cuda.zeros(2048, dtype=torch_cuda.float32, device="cuda")
    out = torch_cuda.full((2, 64), 7.0, dtype=torch_cuda.float32, device="cuda")
    with pytest.raises(L.DspError) as e:  # an all-zero excitation: refused, nothing written
        d.deconvolve(rec, zero, ir_len=64, out=out)
    assert e.value.status == -1 and bool((out == 7.0).all())
    with pytest.raises(L.DspError) as e:  # ir rows inside rec
        d.deconvolve(rec, rec[0] + 1, ir_len=64, out=rec[:, 100:164])
    assert e.value.status == -1
    ref = rec[0].clone()
    with pytest.raises(L.DspError) as e:  # ir row inside ref
        d.deconvolve(rec[:1], ref, ir_len=64, out=ref[None, :64])
    assert e.value.status == -1
    with pytest.raises(L.DspError) as e:  # rfft: the spectrum over its input
        big = torch_cuda.zeros((1, 4096), dtype=torch_cuda.float32, device="cuda")
        d.rfft(big[:, :1024], 1024, out=big[:, 512:512 + 1026])
    assert e.value.status == -1


def test_no_sync_is_stream_ordered(torch_cuda):
    """Without DSP_EXEC_SYNC the calls are ordered by their stream: results after a synchronise are the same bits."""
    n = 1 << 13
    x, spec0, back0 = spectrum_run(n)
    t = torch_cuda.from_numpy(np.array(x)).cuda()
    spec = d.rfft(t, n)
    back = d.irfft(spec, n)
    i = DEC_IDS.index("noise-past-pow2")
    rec, ref, got0, _ = dec_run(i)
    k = du.DEC_CASES[i]
    got = d.deconvolve(torch_cuda.from_numpy(rec).cuda(), torch_cuda.from_numpy(ref).cuda(), ir_len=k["ir_len"],
                       eps=k["eps"], pre=k["pre"])
    torch_cuda.cuda.synchronize()
    assert ru.same_bits(spec.cpu().numpy(), spec0) and ru.same_bits(back.cpu().numpy(), back0)
    assert ru.same_bits(got.cpu().numpy(), got0)
