"""dsp_pvoc, dsp_time_stretch and the pitch shift on the GPU (pvoc.hip) against
the float64 models of tools/pvoc_model.py (tests/pvocutil.py: the cases, the
references, computed once, PVOC_TOL and STRETCH_TOL), against closed forms,
against themselves bit for bit, on unaligned, strided and guarded rows, and
under capture."""
import ctypes as C
import functools

import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L
import cstftutil as cu
import pvocutil as pu
import pvoc_model as pm
import rowsutil as ru

pytestmark = pytest.mark.gpu

N, K = pu.N, pu.K


def gpu_pvoc(Z, rate):
    import torch
    return d.phase_vocoder(torch.from_numpy(np.array(Z)).cuda(), rate).cpu().numpy()


@functools.lru_cache(maxsize=None)
def case_run(case):
    out = gpu_pvoc(pu.make_spectrum(case), case.rate)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("case", pu.CASES, ids=pu.case_id)
def test_parity_with_float64(torch_cuda, case):
    """Every bin of every frame: |Z' - Z'64| <= PVOC_TOL sqrt(t + 1) |Z'64| + ulp32(frame peak)."""
    got, want = case_run(case), pu.reference(case)
    assert got.shape == want.shape == (case.C, d.pvoc_plan(case.F, case.rate, case.C)["frames"], K)
    assert got.dtype == np.complex64 and d.pvoc_plan(case.F, case.rate)["chunk"] == pu.CHUNK
    ru.assert_finite(got.view(np.float32))
    r = pm.ratio(got, want)
    print(f"pvoc ratio {pu.case_id(case)} {r:.3e}")
    assert r <= pu.PVOC_TOL


def test_rate_one_is_the_identity(torch_cuda):
    """No bin is 0, so the increments telescope: Z' = Z within the tolerance at frame t, and
    |Z'| = |Z| to a few float32 ulps (one root, cos^2 + sin^2 within 2^-23 of 1)."""
    Z = pu.random_spectrum(9, 2, 77, zeros=False)
    got = gpu_pvoc(Z, 1.0)
    assert got.shape == Z.shape
    r = pm.ratio(got, Z.astype(np.complex128))
    print(f"rate 1 ratio {r:.3e}")
    assert r <= pu.PVOC_TOL
    m = np.abs(Z.astype(np.complex128))
    assert np.all(np.abs(np.abs(got.astype(np.complex128)) - m) <= 4 * np.spacing(m.astype(np.float32)))


@pytest.mark.parametrize("rate", [0.5, 1.2599])
def test_closed_form_tones(torch_cuda, rate):
    """One bin-centred tone per bin 1, 1001, 4095 at hop 512, A e^(i (phi + 2 pi k0 H f / N)) --
    advances of 1/16, 9/16 and 15/16 of a turn, no quarter turns -- and a real bin 0 of
    alternating sign.  Against pvoc64 of the same float32 spectrogram the bare tolerance holds;
    against the closed form, the same expression in t wherever f + 1 is a frame, the bound is
    that tolerance plus pvoc64's own distance from the closed form (the float32 rounding of the
    spectrogram, computed here, not estimated)."""
    F, H, ks = 12, 512, (1, 1001, 4095)
    Z = pm.tone_spectrogram(F, ks, H, amp=0.75)
    Z[0, :, 0] = pm.real_bin_spectrogram(F)[0, :, 0]
    got, want = gpu_pvoc(Z, rate), pm.pvoc64(Z, rate)
    r = pm.ratio(got, want)
    print(f"tones at rate {rate}: ratio {r:.3e}")
    assert r <= pu.PVOC_TOL
    got, want = got[0], want[0]
    f, _ = pm.positions(F, rate)
    T = int(np.count_nonzero(f + 1 < F))
    t = np.arange(T)
    for k0 in ks:
        exact = pm.tone_expected(T, k0, H, amp=0.75)
        bound = 0.75 * pu.PVOC_TOL * np.sqrt(t + 1) + np.spacing(np.float32(0.75)) + np.abs(want[:T, k0] - exact)
        assert np.all(np.abs(got[:T, k0] - exact) <= bound)
        assert np.max(np.abs(want[:T, k0] - exact)) <= 0.75 * 2.0 ** -20  # (the model does follow the closed form)
    # the real bin: half turns are exact words, so the sign and the +-0 imaginary part are exact
    assert np.array_equal(np.sign(got[:T, 0].real), 1 - 2 * (t % 2)) and not got[:T, 0].imag.any()
    assert np.max(np.abs(np.abs(got[:T, 0].real) - 0.75)) <= 2 * np.spacing(np.float32(0.75))
    others = np.ones(K, bool)
    others[[0, *ks]] = False
    assert not np.ascontiguousarray(got[:, others]).view(np.float32).any()


# ---------------------------------------------------------------------------
# bits: the integer scan
# ---------------------------------------------------------------------------
def test_prefix_frames_have_the_same_bits(torch_cuda):
    """The frames whose f + 1 lies inside a prefix of the input, a count that crosses the
    chunk seam, are bit for bit those of the call on the whole input."""
    F, Fp, rate = 60, 56, 0.8
    Z = pu.random_spectrum(F, 2, 31)
    f, _ = pm.positions(F, rate)
    T1 = int(np.count_nonzero(f + 1 < Fp))
    assert pu.CHUNK < T1 <= d.pvoc_plan(Fp, rate)["frames"] < d.pvoc_plan(F, rate)["frames"]
    whole, part = gpu_pvoc(Z, rate), gpu_pvoc(Z[:, :Fp], rate)
    assert ru.same_bits(whole[:, :T1], part[:, :T1])


def test_two_calls_same_bits(torch_cuda):
    assert ru.same_bits(gpu_pvoc(pu.make_spectrum(pu.SEAM), pu.SEAM.rate), case_run(pu.SEAM))


def test_channel_bits_do_not_depend_on_C(torch_cuda):
    case = pu.CASES[6]
    assert case.C == pu.MAXCH + 1
    Z, out = pu.make_spectrum(case), case_run(case)
    for c in (0, pu.MAXCH - 1, pu.MAXCH):
        assert ru.same_bits(gpu_pvoc(Z[c:c + 1], case.rate)[0], out[c])


def test_host_rows_same_bits(torch_cuda):
    Zh = np.ascontiguousarray(pu.make_spectrum(pu.SEAM))
    out = d.phase_vocoder(Zh, pu.SEAM.rate)
    assert isinstance(out, np.ndarray) and out.dtype == np.complex64 and ru.same_bits(out, case_run(pu.SEAM))


def test_scaling_by_two_is_exact(torch_cuda):
    def twice(z):  # as floats: a complex product with 2 + 0 i would turn a -0 part into +0
        return (np.float32(2) * np.ascontiguousarray(z).view(np.float32)).view(np.complex64)

    assert ru.same_bits(gpu_pvoc(twice(pu.make_spectrum(pu.SEAM)), pu.SEAM.rate), twice(case_run(pu.SEAM)))


def test_silence_gives_positive_zeros(torch_cuda):
    out = gpu_pvoc(np.zeros((2, 70, K), np.complex64), 0.8)
    assert out.shape == (2, 88, K) and not out.view(np.uint32).any()


# ---------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------
def _even(off):
    """A spectrum row must be 8-byte aligned: 2 floats past a 16-byte boundary where the layout has an offset."""
    return 2 if np.any(np.asarray(off) != 0) else 0


@pytest.mark.parametrize("layout", ru.FEW + ("odd_stride",))
def test_row_layouts(torch_cuda, layout):
    """ld_in = 8194 + 6 and ld_out = 8194 + 10 with NaN in the padding and in the guards between
    rows: the dense call's bits, every bin written, nothing else touched, no padding read."""
    torch = torch_cuda
    case = pu.Case(7, 0.8, 3)
    Z = pu.random_spectrum(case.F, case.C, 41)
    Fo = d.pvoc_plan(case.F, case.rate, case.C)["frames"]
    in_off, out_off, stride_mod = ru.LAYOUTS[layout]
    ld_in, ld_out = 2 * K + 6, 2 * K + 10
    padded = np.full((case.C, case.F, ld_in), np.nan, np.float32)
    padded[:, :, :2 * K] = Z.view(np.float32)
    rin = ru.Rows(case.C, case.F * ld_in, _even(in_off), 2 * stride_mod, torch)
    rin.fill(padded.reshape(case.C, -1))
    rout = ru.Rows(case.C, Fo * ld_out, _even(out_off), 2 * stride_mod, torch)
    sp, ex = L.dsp_pvoc_spec(case.rate), d.api._exec(rin.view, 0, None)
    L.check(L.lib().dsp_pvoc(L.chan_table(rin.ptrs()), case.C, case.F, ld_in, L.chan_table(rout.ptrs()), ld_out,
                             C.byref(sp), C.byref(ex)), "dsp_pvoc")
    torch.cuda.synchronize()
    rout.check_output(Fo * ld_out, 2 * K, ld_out)
    got = rout.numpy().reshape(case.C, Fo, ld_out)[:, :, :2 * K]
    ru.assert_finite(got)
    assert ru.same_bits(np.ascontiguousarray(got), gpu_pvoc(Z, case.rate).view(np.float32))


def test_refusals_write_nothing(torch_cuda):
    torch = torch_cuda
    F, rate = 4, 0.5
    Fo = d.pvoc_plan(F, rate)["frames"]
    Zt = torch.full((2, F * 2 * K), 7.0, dtype=torch.float32, device="cuda")
    Wt = torch.full((2, Fo * 2 * K + 8), 3.0, dtype=torch.float32, device="cuda")
    ex = d.api._exec(Zt, 0, None)
    off_ex = d.api._exec(Zt, 4096, None)
    rows = lambda t, off=0: L.chan_table([t[c].data_ptr() + off for c in range(2)])  # noqa: E731
    lib, PS, I = L.lib(), L.dsp_pvoc_spec, L.DSP_ERR_INVALID

    def pv(in_=None, C_=2, F_=F, ld_in=2 * K, out=None, ld_out=2 * K, sp=PS(rate), ex_=ex):
        return lib.dsp_pvoc(rows(Zt) if in_ is None else in_, C_, F_, ld_in, rows(Wt) if out is None else out, ld_out,
                            C.byref(sp) if sp is not None else None, C.byref(ex_))

    for call in (lambda: pv(C_=0), lambda: pv(F_=0), lambda: pv(sp=None), lambda: pv(sp=PS(0.12)), lambda: pv(sp=PS(8.5)),
                 lambda: pv(sp=PS(float("nan"))), lambda: pv(sp=PS(float("inf"))),
                 lambda: pv(ld_in=2 * K + 1), lambda: pv(ld_in=2 * K - 2), lambda: pv(ld_out=2 * K + 1),
                 lambda: pv(ld_out=2 * K - 2), lambda: pv(ex_=off_ex),
                 lambda: pv(in_=rows(Zt, 4)), lambda: pv(out=rows(Wt, 4)),
                 lambda: pv(in_=L.chan_table([0, 0])), lambda: pv(out=L.chan_table([Wt[0].data_ptr(), 0])),
                 lambda: pv(out=L.chan_table([Wt[0].data_ptr()] * 2)), lambda: pv(out=rows(Wt, 16), in_=rows(Wt)),
                 lambda: pv(out=L.chan_table([Wt[0].data_ptr(), Zt[1].data_ptr() + 64]))):
        assert call() == I
    torch.cuda.synchronize()
    assert torch.all(Zt == 7.0) and torch.all(Wt == 3.0)
    assert pv() == L.DSP_OK


def test_capture_replays_the_eager_bits(torch_cuda):
    """After one eager call of the same shape on the capturing stream (the scratch is kept per
    stream) the three launches record into a graph; a replay gives the eager bits."""
    torch = torch_cuda
    Zt = torch.from_numpy(np.array(pu.make_spectrum(pu.SEAM))).cuda()
    want = d.phase_vocoder(Zt, pu.SEAM.rate)
    out = torch.zeros_like(want)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d.phase_vocoder(Zt, pu.SEAM.rate, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        d.phase_vocoder(Zt, pu.SEAM.rate, out=out)
    out.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


# ---------------------------------------------------------------------------
# dsp_time_stretch and the pitch shift
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", pu.STRETCH_CASES, ids=pu.stretch_id)
def test_time_stretch_against_the_float64_chain(torch_cuda, case):
    """Sums of bin-centred tones of comparable level (no occupied bin is weak) against stft64,
    pvoc64, istft64 in dsp_istft's shape; the default length is the plan's."""
    import torch
    x = torch.from_numpy(np.array(pu.stretch_input(case))).cuda()
    p = d.time_stretch_plan(pu.stretch_len(case), case.rate, case.C, case.H)
    assert p["frames_in"] == case.F and p["frames_out"] == pm.frames_out(case.F, case.rate)
    assert p["Lout"] == min(p["Lout_full"], round(pu.stretch_len(case) / case.rate))
    y = d.time_stretch(x, case.rate, case.H, length=p["Lout_full"])
    assert torch.is_tensor(y) and y.dtype == torch.float32 and tuple(y.shape) == (case.C, p["Lout_full"])
    yn = y.cpu().numpy()
    ru.assert_finite(yn)
    r = pu.stretch_ratio(yn, case)
    print(f"stretch ratio {pu.stretch_id(case)} {r:.3e}")
    assert r <= pu.STRETCH_TOL
    # the default length, and host rows: the same bits
    yd = d.time_stretch(x, case.rate, case.H)
    assert tuple(yd.shape) == (case.C, p["Lout"]) and torch.equal(yd, y[:, :p["Lout"]])
    yh = d.time_stretch(np.ascontiguousarray(pu.stretch_input(case)), case.rate, case.H)
    assert isinstance(yh, np.ndarray) and ru.same_bits(yh, yd.cpu().numpy())


@pytest.mark.parametrize("rate", [0.8, 1.25])
def test_time_stretch_of_one_tone_is_the_tone(torch_cuda, rate):
    """A bin-centred tone's bins all advance by the tone's own phase per frame (k0 H / N =
    187.6875 turns here), so the output is the same tone, Lout long: checked on the samples
    that only frames with f + 1 < F reach (the later ones fade against the zero pad) and with
    den >= 2 floor (the Hann floor band of cstftutil aside).  Against the float64 chain the
    bare STRETCH_TOL holds; against the tone the bound is that plus the float64 chain's own
    distance from the tone, computed here."""
    import torch
    F, H, k0, amp, phi = 9, 1536, 1001, 0.5, 0.4
    x = pu.tones(N + (F - 1) * H, (k0,), (amp,), (phi,))[None]
    p = d.time_stretch_plan(x.shape[1], rate, 1, H)
    y = d.time_stretch(torch.from_numpy(x).cuda(), rate, H, length=p["Lout_full"]).cpu().numpy()[0]
    y64 = pm.stretch64(x, rate, H, "hann", None, 0.0)[0]
    f, _ = pm.positions(F, rate)
    lim = int(np.count_nonzero(f + 1 < F)) * H
    env = cu.envelope(p["frames_out"], H, "hann")
    ok = env.hi[:lim]
    A = env.A[:lim][ok]
    tone = amp * np.cos(2 * np.pi * k0 * np.arange(lim) / N + phi)
    scale = np.max(np.abs(y64))
    e64 = np.abs(y[:lim] - y64[:lim])[ok] / (A * scale)
    print(f"one tone at rate {rate}: against the float64 chain {e64.max():.3e}")
    assert lim > N and e64.max() <= pu.STRETCH_TOL
    model = np.abs(y64[:lim] - tone)[ok]
    assert np.all(np.abs(y[:lim] - tone)[ok] <= pu.STRETCH_TOL * A * scale + model)
    assert model.max() <= amp * 2.0 ** -20  # (the float64 chain does return the tone)


def test_pitch_shift(torch_cuda):
    """A bin-centred tone at k0 moves to k0 p / q; the length comes back within a sample; the
    call is its two public halves composed, bit for bit."""
    import torch
    F, H, k0, st = 9, 2048, 1000, 3
    Lx = N + (F - 1) * H
    x = torch.from_numpy(pu.tones(Lx, (k0,), (0.5,), (0.2,))[None]).cuda()
    p, q = d.pitch_ratio(st)
    y = d.pitch_shift(x, st)
    assert torch.is_tensor(y) and y.dtype == torch.float32 and y.shape[0] == 1 and abs(y.shape[1] - Lx) <= 1
    pl = d.pitch_shift_plan(Lx, st)
    assert (pl["p"], pl["q"]) == (p, q) and pl["stretched"] == (2 * Lx * p + q) // (2 * q) and y.shape[1] == pl["Lout"]
    assert pl["padded"] >= Lx and d.time_stretch_plan(pl["padded"], q / p)["Lout_full"] >= pl["stretched"]
    xp = torch.nn.functional.pad(x, (0, pl["padded"] - Lx))
    by_hand = d.resample(d.time_stretch(xp, q / p, H, "hann", length=pl["stretched"]), p, q)
    assert torch.equal(y, by_hand)
    mag = d.stft_magnitude(y, 8192, H, d.DSP_WIN_HANN).cpu().numpy()[0, :, :K]
    assert mag.shape[0] >= 3 and np.all(np.argmax(mag[1:-1], axis=1) == round(k0 * p / q))
    down = d.pitch_shift(x, -2)
    p2, q2 = d.pitch_ratio(-2)
    assert abs(down.shape[1] - Lx) <= 1
    m2 = d.stft_magnitude(down, 8192, H, d.DSP_WIN_HANN).cpu().numpy()[0, :, :K]
    assert np.all(np.argmax(m2[1:-1], axis=1) == round(k0 * p2 / q2))


def test_pitch_shift_at_a_rounding_tie(torch_cuda):
    """An octave down of an odd length: L / 2 is a tie, and the one rule, floor(x + 1 / 2), is
    the plan's, so the Python face and its own composition agree."""
    import torch
    Lx = N + 8 * 2048 + 1
    pl = d.pitch_shift_plan(Lx, -12)
    assert (pl["p"], pl["q"], pl["stretched"], pl["padded"]) == (1, 2, (Lx + 1) // 2, Lx)
    x = torch.from_numpy(pu.tones(Lx, (1000,), (0.5,), (0.2,))[None]).cuda()
    y = d.pitch_shift(x, -12)
    assert y.shape[1] == pl["Lout"] and abs(pl["Lout"] - Lx) <= 1
    assert torch.equal(y, d.resample(d.time_stretch(x, 2.0, length=pl["stretched"]), 1, 2))


def test_debug_hooks_keep_the_bits(torch_cuda):
    """DSP_DEBUG_PVOC_CHUNK cuts the integer sum elsewhere and variant 4 stores the increments:
    neither changes a bit; variants 1 and 2 stay inside the tolerance."""
    lib, case, want = L.lib(), pu.SEAM, case_run(pu.SEAM)
    try:
        for chunk in (8, 33, 4096):
            L.check(lib.dsp_debug_set(7, chunk), "dsp_debug_set")
            assert d.pvoc_plan(case.F, case.rate)["chunk"] == chunk
            assert ru.same_bits(gpu_pvoc(pu.make_spectrum(case), case.rate), want)
        L.check(lib.dsp_debug_set(7, 0), "dsp_debug_set")
        L.check(lib.dsp_debug_set(8, 4), "dsp_debug_set")
        assert ru.same_bits(gpu_pvoc(pu.make_spectrum(case), case.rate), want)
        for variant in (1, 2, 3):
            L.check(lib.dsp_debug_set(8, variant), "dsp_debug_set")
            assert pm.ratio(gpu_pvoc(pu.make_spectrum(case), case.rate), pu.reference(case)) <= pu.PVOC_TOL
        assert lib.dsp_debug_set(7, 7) == L.DSP_ERR_INVALID and lib.dsp_debug_set(8, 8) == L.DSP_ERR_INVALID
    finally:
        lib.dsp_debug_set(7, 0)
        lib.dsp_debug_set(8, 0)
    assert d.pvoc_plan(case.F, case.rate)["chunk"] == pu.CHUNK
