"""dsp_stft and dsp_istft on the GPU (stft_cx.hip) against the float64 models of
tools/stft_model.py (tests/cstftutil.py: the cases, the references, computed
once, STFT_TOL and ISTFT_TOL), against closed forms, against the shipped STFT
and Welch sums, against themselves bit for bit, on unaligned, strided and
guarded rows, through the Python face against torch.stft, and under capture."""
import ctypes as C
import functools

import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L
import cstftutil as cu
import rowsutil as ru
import stft_model as sm
import stftutil as su
import welchutil as wu

pytestmark = pytest.mark.gpu

N, K = cu.N, cu.K


def gpu_stft(x, H, window):
    import torch
    return d.stft(torch.from_numpy(np.array(x)).cuda(), H, window).cpu().numpy()


def gpu_istft(Z, H, window, length=None):
    import torch
    return d.istft(torch.from_numpy(np.array(Z)).cuda(), H, window, length).cpu().numpy()


@functools.lru_cache(maxsize=None)
def forward_run(case):
    X = gpu_stft(cu.make_input(case), case.H, case.window)
    X.setflags(write=False)
    return X


@pytest.mark.parametrize("case", cu.FORWARD, ids=cu.case_id)
def test_forward_parity_with_float64(torch_cuda, case):
    """Per frame max_k |X - X64| <= STFT_TOL max_k |X64|; bins 0 and 4096 real, +0."""
    X, want = forward_run(case), cu.forward_reference(case)
    assert X.shape == (case.C, case.F, K) and X.dtype == np.complex64
    assert d.stft_plan(cu.case_len(case), case.C, case.H, case.window)["frames"] == case.F
    ru.assert_finite(X.view(np.float32))
    r = sm.ratios(X, want)
    print(f"stft ratio {cu.case_id(case)} {r:.3e}")
    assert r <= cu.STFT_TOL
    for k in (0, K - 1):
        assert not X[..., k].imag.any() and not np.signbit(X[..., k].imag).any()


@pytest.mark.parametrize("case", cu.INVERSE, ids=cu.case_id)
def test_inverse_parity_of_arbitrary_spectra(torch_cuda, case):
    """Seeded complex noise with imaginary parts in bins 0 and 4096: per row
    max_i |y - y64| / A[i] <= ISTFT_TOL max_f max |v_f| where den >= 2 floor, exactly 0
    where den < floor / 2, one or the other in the band between."""
    Z, ref, env = cu.make_spectrum(case), cu.inverse_reference(case), cu.envelope(case.F, case.H, case.window)
    p = d.istft_plan(case.F, case.C, case.H, case.window)
    assert p["Lout"] == env.den.size
    y = gpu_istft(Z, case.H, case.window)
    assert y.shape == (case.C, p["Lout"]) and y.dtype == np.float32
    ru.assert_finite(y)
    r = cu.inverse_ratio(y, ref.q, env, ref.vmax)
    print(f"istft ratio {cu.case_id(case)} {r:.3e}")
    assert r <= cu.ISTFT_TOL


@pytest.mark.parametrize("case", cu.ROUND_TRIP, ids=cu.case_id)
def test_round_trip(torch_cuda, case):
    """|istft(stft(x))[i] - x[i]| <= (STFT_TOL + ISTFT_TOL) A[i] max |x| wherever den >= 2 floor."""
    import torch
    x, env = cu.make_input(case), cu.envelope(case.F, case.H, case.window)
    Zt = d.stft(torch.from_numpy(np.array(x)).cuda(), case.H, case.window)
    y = d.istft(Zt, case.H, case.window).cpu().numpy()
    n = env.den.size
    assert y.shape == (case.C, n)
    r = cu.inverse_ratio(y, x[:, :n].astype(np.float64), env, np.max(np.abs(x), axis=1).astype(np.float64))
    print(f"round trip ratio {cu.case_id(case)} {r:.3e}")
    assert r <= cu.STFT_TOL + cu.ISTFT_TOL


# ---------------------------------------------------------------------------
# closed forms (stftutil.py's generators): the phase, not only the magnitude
# ---------------------------------------------------------------------------
def _sparse_complex(window, J, A):
    """sum_m A[f, m] w[J[f, m]] exp(-2 i pi k J[f, m] / N): [F, K] complex128 over the float table."""
    w = sm.window_table(window).astype(np.float64)
    tab = np.exp(-2j * np.pi * np.arange(N) / N)
    k = np.arange(K, dtype=np.int64)
    z = np.zeros((J.shape[0], K), complex)
    for m in range(J.shape[1]):
        z += (A[:, m] * w[J[:, m]])[:, None] * tab[(J[:, m, None] * k[None, :]) % N]
    return z


def _check_sparse(X, window, J, A, what):
    """every bin within STFT_TOL of the largest magnitude impulses of those amplitudes can produce"""
    want = _sparse_complex(window, J, A)
    bar = cu.STFT_TOL * np.abs(A).sum(axis=1) * float(sm.window_table(window).max())
    worst = np.max(np.max(np.abs(X - want), axis=1) / bar)
    print(f"{what}: worst {worst:.3f} of the bar")
    assert worst <= 1.0


@pytest.mark.parametrize("window", ["hann", "hamming"])
def test_closed_form_impulses(torch_cuda, window):
    """An impulse at p of frame f: X_f[k] = a w[p] e^(-2 pi i k p / N), every bin."""
    pos = su.impulse_positions(N)[::7]
    x = su.impulse_frames(N, pos, 0.75)
    X = gpu_stft(x[None, :], N, window)[0]
    _check_sparse(X, window, *su.sparse_cases(pos, [0.75]), f"impulses {window}")


def test_closed_form_impulse_across_hops(torch_cuda):
    """One impulse seen by overlapping frames at hop 513: frame f holds it at p - f H."""
    H, F, p = 513, 9, 4321
    x = np.zeros(N + (F - 1) * H, np.float32)
    x[p] = -0.5
    X = gpu_stft(x[None, :], H, "hamming")[0]
    J = (p - np.arange(F) * H)[:, None]
    assert np.all((J >= 0) & (J < N))
    _check_sparse(X, "hamming", *su.sparse_cases(J, [-0.5]), "impulse across hops")


def test_closed_form_pairs(torch_cuda):
    pairs = su.impulse_pairs(N)[::5]
    x = su.pair_frames(N, pairs, 0.5, -0.25)
    X = gpu_stft(x[None, :], N, "hann")[0]
    _check_sparse(X, "hann", *su.sparse_cases(pairs, [0.5, -0.25]), "pairs")


def test_closed_form_tones(torch_cuda):
    """A bin-centred tone: the float64 STFT of the float32 signal, per frame within STFT_TOL of its peak."""
    bins = su.tone_bins(N)[::3]
    x = su.tone_frames(N, bins)
    X = gpu_stft(x[None, :], N, "hann")
    want = sm.stft64(x[None, :], N, "hann")
    assert sm.ratios(X, want) <= cu.STFT_TOL
    assert np.array_equal(np.argmax(np.abs(X[0]), axis=1), bins)


# ---------------------------------------------------------------------------
# cross-checks against shipped code
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("F,H,window", [(1, 4096, "hann"), (8, 4096, "hamming"), (5, 4095, "hann")])
def test_cross_check_with_stft_magnitude_and_welch(torch_cuda, F, H, window):
    """|X| / sqrt(N) against dsp_stft_magnitude within its documented 1e-6 of the frame's
    peak plus STFT_TOL; sum_f |X|^2 in float64 against dsp_welch's sxx within WELCH_TOL
    max sxx plus the squared forward bound N-free: 2 m d + d^2 with d = STFT_TOL m."""
    import torch
    x, _ = wu.make_signals(N + (F - 1) * H + H - 1, 2, seed=7)
    tx = torch.from_numpy(x).cuda()
    X = d.stft(tx, H, window).cpu().numpy().astype(np.complex128)
    win = d.DSP_WIN_HANN if window == "hann" else d.DSP_WIN_HAMMING
    mag = d.stft_magnitude(tx, 8192, H, win).cpu().numpy().astype(np.float64)[:, :, :K]
    a = np.abs(X) / np.sqrt(N)
    peak = a.max(axis=2)
    assert np.all(np.max(np.abs(a - mag), axis=2) <= (1e-6 + cu.STFT_TOL) * peak + su.ABS_FLOOR)
    sxx = d.welch_sums(tx, None, H, window)[0].cpu().numpy()
    via = np.sum(np.abs(X) ** 2, axis=1)
    m = np.abs(X).max(axis=2)  # per (channel, frame)
    bound = wu.WELCH_TOL * sxx.max(axis=1) + np.sum((2 * cu.STFT_TOL + cu.STFT_TOL ** 2) * m * m, axis=1)
    assert np.all(np.max(np.abs(sxx - via), axis=1) <= bound)


# ---------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------
CASE_BITS = cu.Case(6, 2730, 3, "hann", "noise", True, True)


def test_two_calls_same_bits(torch_cuda):
    x, Z = cu.make_input(CASE_BITS), cu.make_spectrum(CASE_BITS)
    assert ru.same_bits(gpu_stft(x, 2730, "hann"), forward_run(CASE_BITS))
    assert ru.same_bits(gpu_istft(Z, 2730, "hann"), gpu_istft(Z, 2730, "hann"))


def test_channel_bits_do_not_depend_on_C(torch_cuda):
    """Channel c alone and inside kMaxChannels + 1 channels (two groups): the same bits, both ways."""
    case = next(c for c in cu.FORWARD if c.C == cu.MAXCH + 1 and c.window == "hann" and c.signal == "noise")
    x, X = cu.make_input(case), forward_run(case)
    for c in (0, cu.MAXCH - 1, cu.MAXCH):
        assert ru.same_bits(gpu_stft(x[c:c + 1], case.H, case.window)[0], X[c])
    Z = np.ascontiguousarray(np.broadcast_to(cu.make_spectrum(CASE_BITS)[:1], (cu.MAXCH + 1, 6, K))) * \
        (1 + np.arange(cu.MAXCH + 1, dtype=np.float32))[:, None, None]
    y = gpu_istft(Z, 2730, "hann")
    for c in (0, cu.MAXCH - 1, cu.MAXCH):
        assert ru.same_bits(gpu_istft(Z[c:c + 1], 2730, "hann")[0], y[c])


def test_host_rows_same_bits(torch_cuda):
    x, Z = np.ascontiguousarray(cu.make_input(CASE_BITS)), np.ascontiguousarray(cu.make_spectrum(CASE_BITS))
    Xh = d.stft(x, 2730, "hann")
    assert isinstance(Xh, np.ndarray) and ru.same_bits(Xh, forward_run(CASE_BITS))
    yh = d.istft(Z, 2730, "hann")
    assert isinstance(yh, np.ndarray) and ru.same_bits(yh, gpu_istft(Z, 2730, "hann"))


def test_scaling_by_two_is_exact(torch_cuda):
    x = cu.make_input(CASE_BITS)
    assert ru.same_bits(gpu_stft(2.0 * x, 2730, "hann"), 2.0 * forward_run(CASE_BITS))


def test_silence_gives_zeros(torch_cuda):
    X = gpu_stft(np.zeros((2, 3 * N), np.float32), 4095, "hamming")
    assert X.shape == (2, 5, K) and not X.view(np.float32).any()
    y = gpu_istft(np.zeros((2, 5, K), np.complex64), 4095, "hamming")
    assert y.shape == (2, N + 4 * 4095) and not y.any()


# ---------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------
def _spec(H, window, floor=None):
    w = d.api._stft_window(window)
    return L.dsp_stft_spec(8192, H, w) if floor is None else L.dsp_istft_spec(8192, H, w, floor)


def _even(off):
    """A spectrum row must be 8-byte aligned: 2 floats past a 16-byte boundary where the layout has an offset."""
    return 2 if np.any(np.asarray(off) != 0) else 0


@pytest.mark.parametrize("layout", ru.FEW + ("odd_stride",))
def test_row_layouts_forward(torch_cuda, layout):
    """ld = 8194 + 6 with NaN in the padding and in the guards between rows, input rows 4
    bytes past a 16-byte boundary or strided, NaN after the L samples: the dense call's
    bits, every bin written, nothing else touched."""
    torch = torch_cuda
    case = cu.Case(5, 4095, 3, "hann", "noise", True, True)
    Lx = cu.case_len(case)
    x = wu.make_signals(Lx, case.C, seed=11)[0]
    in_off, out_off, stride_mod = ru.LAYOUTS[layout]
    rin = ru.Rows(case.C, Lx + 5, in_off, stride_mod, torch).fill(x, Lx)
    ld = 2 * K + 6
    rout = ru.Rows(case.C, case.F * ld, _even(out_off), 2 * stride_mod, torch)
    sp, ex = _spec(case.H, case.window), d.api._exec(rin.view, 0, None)
    L.check(L.lib().dsp_stft(L.chan_table(rin.ptrs()), case.C, Lx, L.chan_table(rout.ptrs()), ld, C.byref(sp),
                             C.byref(ex)), "dsp_stft")
    torch.cuda.synchronize()
    rout.check_output(case.F * ld, 2 * K, ld)
    got = rout.numpy().reshape(case.C, case.F, ld)[:, :, :2 * K]
    ru.assert_finite(got)
    want = gpu_stft(x, case.H, case.window).view(np.float32)
    assert ru.same_bits(np.ascontiguousarray(got), want)


@pytest.mark.parametrize("layout", ru.FEW + ("odd_stride",))
def test_row_layouts_inverse(torch_cuda, layout):
    """The same for dsp_istft, with Lout < Lout_full: nothing is written past Lout."""
    torch = torch_cuda
    case = CASE_BITS
    Z = cu.make_spectrum(case)
    in_off, out_off, stride_mod = ru.LAYOUTS[layout]
    ld = 2 * K + 6
    padded = np.full((case.C, case.F, ld), np.nan, np.float32)
    padded[:, :, :2 * K] = Z.view(np.float32)
    rin = ru.Rows(case.C, case.F * ld, _even(in_off), 2 * stride_mod, torch)
    rin.fill(padded.reshape(case.C, -1))
    full = N + (case.F - 1) * case.H
    Lout = full - 1234
    rout = ru.Rows(case.C, full, out_off, stride_mod, torch)
    sp, ex = _spec(case.H, case.window, 1e-10), d.api._exec(rin.view, 0, None)
    L.check(L.lib().dsp_istft(L.chan_table(rin.ptrs()), case.C, case.F, ld, L.chan_table(rout.ptrs()), Lout,
                              C.byref(sp), C.byref(ex)), "dsp_istft")
    torch.cuda.synchronize()
    rout.check_output(Lout)
    got = rout.numpy(Lout)
    ru.assert_finite(got)
    assert ru.same_bits(got, np.ascontiguousarray(gpu_istft(Z, case.H, case.window)[:, :Lout]))
    assert ru.same_bits(got, gpu_istft(Z, case.H, case.window, Lout))


def test_overlapping_rows_are_refused(torch_cuda):
    torch = torch_cuda
    Lx = 3 * N
    F = 5
    x = torch.full((2, Lx), 0.5, dtype=torch.float32, device="cuda")
    Zt = torch.full((2, F * 2 * K), 7.0, dtype=torch.float32, device="cuda")
    ex = d.api._exec(x, 0, None)
    sp, isp = _spec(4096, "hann"), _spec(4096, "hann", 1e-10)
    rows = lambda t, off=0: L.chan_table([t[c].data_ptr() + off for c in range(2)])  # noqa: E731
    same = L.chan_table([Zt[0].data_ptr(), Zt[0].data_ptr()])
    lib = L.lib()
    assert lib.dsp_stft(rows(x), 2, Lx, rows(x, 8), 2 * K, C.byref(sp), C.byref(ex)) == L.DSP_ERR_INVALID
    assert lib.dsp_stft(rows(x), 2, Lx, same, 2 * K, C.byref(sp), C.byref(ex)) == L.DSP_ERR_INVALID
    assert lib.dsp_stft(rows(x), 2, Lx, rows(Zt, 4), 2 * K, C.byref(sp), C.byref(ex)) == L.DSP_ERR_INVALID  # misaligned
    assert lib.dsp_istft(rows(Zt), 2, F, 2 * K, rows(Zt, 16), 100, C.byref(isp), C.byref(ex)) == L.DSP_ERR_INVALID
    assert lib.dsp_istft(rows(Zt), 2, F, 2 * K, L.chan_table([x[0].data_ptr()] * 2), 100, C.byref(isp),
                         C.byref(ex)) == L.DSP_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.all(x == 0.5) and torch.all(Zt == 7.0)
    assert lib.dsp_stft(rows(x), 2, Lx, rows(Zt), 2 * K, C.byref(sp), C.byref(ex)) == L.DSP_OK


# ---------------------------------------------------------------------------
# the Python face, and capture
# ---------------------------------------------------------------------------
def test_python_face_against_torch(torch_cuda):
    """Shape and dtype as documented on torch CUDA tensors and on numpy; stft equals
    torch.stft(..., center=False) transposed within STFT_TOL of each frame's peak."""
    torch = torch_cuda
    H = 2048
    x = cu.make_input(CASE_BITS)[:2, :N + 4 * H + 99]
    tx = torch.from_numpy(np.array(x)).cuda()
    Z = d.stft(tx, hop=H, window="hamming")
    assert torch.is_tensor(Z) and Z.is_cuda and Z.dtype == torch.complex64 and tuple(Z.shape) == (2, 5, K)
    w = torch.from_numpy(sm.window_table("hamming")).cuda()
    T = torch.stft(tx, N, H, window=w, center=False, return_complex=True).transpose(1, 2)
    err = (Z - T).abs().amax(dim=2) / T.abs().amax(dim=2)
    print(f"stft against torch.stft {float(err.max()):.3e}")
    assert float(err.max()) <= cu.STFT_TOL
    y = d.istft(Z, hop=H, window="hamming", length=N + 4 * H - 7)
    assert torch.is_tensor(y) and y.dtype == torch.float32 and tuple(y.shape) == (2, N + 4 * H - 7)
    Zn = d.stft(np.ascontiguousarray(x), hop=H, window="hamming")
    assert isinstance(Zn, np.ndarray) and Zn.dtype == np.complex64 and ru.same_bits(Zn, Z.cpu().numpy())
    yn = d.istft(Zn, hop=H, window="hamming")
    assert isinstance(yn, np.ndarray) and yn.dtype == np.float32 and yn.shape == (2, N + 4 * H)
    assert ru.same_bits(np.ascontiguousarray(yn[:, :y.shape[1]]), y.cpu().numpy())
    out = torch.empty((2, 5, K), dtype=torch.complex64, device="cuda")
    assert d.stft(tx, hop=H, window="hamming", out=out) is out and torch.equal(out, Z)


def test_capture_replays_the_eager_bits(torch_cuda):
    """After one eager call of the same shape on the capturing stream (the scratch is kept
    per stream) both calls record into one graph, a linear chain on one stream; a replay
    gives the eager bits."""
    torch = torch_cuda
    case = CASE_BITS
    tx = torch.from_numpy(np.array(cu.make_input(case))).cuda()
    Z0 = d.stft(tx, case.H, case.window)
    y0 = d.istft(Z0, case.H, case.window)
    Z, y = torch.zeros_like(Z0), torch.zeros_like(y0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # the eager call of this shape on the capture stream
        d.stft(tx, case.H, case.window, out=Z)
        d.istft(Z, case.H, case.window, out=y)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        d.stft(tx, case.H, case.window, out=Z)
        d.istft(Z, case.H, case.window, out=y)
    Z.zero_()
    y.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(Z, Z0) and torch.equal(y, y0)
