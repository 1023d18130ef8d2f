"""dsp_welch on the GPU (welch.hip) against the float64 model of
tools/welch_model.py (tests/welchutil.py: the cases, the references, computed
once, and WELCH_TOL), against itself, against the shipped STFT, on unaligned,
strided and guarded rows, and through the Python face against scipy."""
import functools

import numpy as np
import pytest

import dspbench as d
import rowsutil as ru
import welchutil as wu
import welch_model as wm

pytestmark = pytest.mark.gpu

K = wu.K


def gpu_sums(x, ref, H, window):
    """dsp_welch on device rows -> numpy (sxx, srr, sxy interleaved)."""
    import torch
    tx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    tr = None if ref is None else torch.from_numpy(np.ascontiguousarray(ref)).cuda()
    return tuple(None if a is None else a.cpu().numpy() for a in d.welch_sums(tx, tr, H, window))


@functools.lru_cache(maxsize=None)
def case_run(case):
    x, ref = wu.make_case(case)
    out = gpu_sums(x, ref, case.H, case.window)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("case", wu.CASES, ids=wu.case_id)
def test_parity_with_float64(torch_cuda, case):
    """Per row max_k |S - S64| <= WELCH_TOL max_k S64 (sxy: sqrt(max sxx max srr))."""
    got, want = wu.as_model(*case_run(case)), wu.reference(case)
    assert d.welch_plan(wu.case_len(case), case.C, case.ref, case.H, case.window)["frames"] == case.F
    r = wm.ratios(got, want)
    print(f"welch ratio {wu.case_id(case)} {r}")
    ru.assert_finite(*[a for a in got if a is not None])
    assert (got[1] is None) == (not case.ref) and (got[2] is None) == (not case.ref)
    for kind, v in r.items():
        assert v <= wu.WELCH_TOL, (kind, v)


CASE_REF = wu.Case(wu.RUN + 1, 2730, 2, "hann", True, "noise")


def test_in_equal_to_ref_has_no_imaginary_part(torch_cuda):
    """conj(R) X with X's bits equal to R's: im = rr xi - ri xr is two equal rounded
    products and their difference -- exactly 0, and re = |R|^2 summed the way srr is not
    (products rounded apart from the sum), so only within the bound (each is within
    WELCH_TOL of the truth)."""
    _, ref = wu.make_case(CASE_REF)
    x = np.stack([ref, ref.copy()])
    sxx, srr, sxy = gpu_sums(x, ref, CASE_REF.H, CASE_REF.window)
    assert np.all(sxy[:, 1::2] == 0.0)
    assert np.all(np.abs(sxy[:, 0::2] - srr) <= 2 * wu.WELCH_TOL * srr.max())
    assert ru.same_bits(sxx[0], srr) and ru.same_bits(sxx[1], srr)


def test_silence_sums_to_zero(torch_cuda):
    L = wu.case_len(CASE_REF)
    sxx, srr, sxy = gpu_sums(np.zeros((2, L), np.float32), np.zeros(L, np.float32), CASE_REF.H, "hamming")
    assert not sxx.any() and not srr.any() and not sxy.any()


def test_two_calls_same_bits(torch_cuda):
    x, ref = wu.make_case(CASE_REF)
    a, b = gpu_sums(x, ref, CASE_REF.H, CASE_REF.window), gpu_sums(x, ref, CASE_REF.H, CASE_REF.window)
    assert all(ru.same_bits(p, q) for p, q in zip(a, b))


def test_channel_bits_do_not_depend_on_C(torch_cuda):
    """Channel c alone and inside kMaxChannels + 1 channels (two groups): the same bits."""
    case = wu.CASES[6]
    assert case.C == wu.MAXCH + 1
    x, ref = wu.make_case(case)
    sxx, srr, sxy = case_run(case)
    for c in (0, wu.MAXCH - 1, wu.MAXCH):
        a = gpu_sums(x[c:c + 1], ref, case.H, case.window)
        assert ru.same_bits(a[0][0], sxx[c]) and ru.same_bits(a[2][0], sxy[c]) and ru.same_bits(a[1], srr)


def test_host_rows_same_bits(torch_cuda):
    x, ref = wu.make_case(CASE_REF)
    dev = gpu_sums(x, ref, CASE_REF.H, CASE_REF.window)
    host = d.welch_sums(np.ascontiguousarray(x), np.ascontiguousarray(ref), CASE_REF.H, CASE_REF.window)
    assert all(ru.same_bits(p, q) for p, q in zip(dev, host))
    dev = gpu_sums(x, None, CASE_REF.H, CASE_REF.window)
    host = d.welch_sums(np.ascontiguousarray(x), None, CASE_REF.H, CASE_REF.window)
    assert host[1] is None and host[2] is None and ru.same_bits(dev[0], host[0])


@pytest.mark.parametrize("F,H,window", [(1, 4096, "hann"), (8, 4096, "hamming"), (5, 4095, "hann")])
def test_cross_check_with_stft_magnitude(torch_cuda, F, H, window):
    """sxx against sum_f (sqrt(N) dsp_stft_magnitude)^2 in float64, within both documented
    bounds: WELCH_TOL max sxx, and the STFT's 1e-6 max_k per frame, which squares to
    N (2 m d + d^2) with d = 1e-6 m."""
    import torch
    x, _ = wu.make_signals(wu.N + (F - 1) * H + H - 1, 2, seed=7)
    sxx = gpu_sums(x, None, H, window)[0]
    win = d.DSP_WIN_HANN if window == "hann" else d.DSP_WIN_HAMMING
    mag = d.stft_magnitude(torch.from_numpy(x).cuda(), 8192, H, win).cpu().numpy().astype(np.float64)
    assert mag.shape[1] == F
    via = np.sum(wu.N * mag[:, :, :K] ** 2, axis=1)
    m = mag.max(axis=2)  # per (channel, frame)
    bound = wu.WELCH_TOL * via.max(axis=1) + np.sum(wu.N * (2e-6 + 1e-12) * m * m, axis=1)
    assert np.all(np.max(np.abs(sxx - via), axis=1) <= bound)


def double_rows(torch, C, n):
    """C float64 rows of n in one NaN-filled allocation with guards between them."""
    G = 16
    whole = torch.full((C * (n + G) + G,), float("nan"), dtype=torch.float64, device="cuda")
    view = whole.as_strided((C, n), (n + G, 1), G)
    mask = np.ones(whole.shape[0], bool)
    for c in range(C):
        mask[G + c * (n + G):G + c * (n + G) + n] = False
    return whole, view, mask


@pytest.mark.parametrize("layout", ru.ALL)
def test_row_layouts(torch_cuda, layout):
    """Unaligned (4-byte) and strided input rows at an odd hop, NaN before and after every
    row: the aligned call's bits, nothing non-finite, and output guards untouched."""
    torch = torch_cuda
    case = wu.Case(3, 4095, 3, "hann", True, "noise")
    L = wu.case_len(case)
    x, ref = wu.make_signals(L, case.C, seed=11)
    in_off, _, stride_mod = ru.LAYOUTS[layout]
    rin = ru.Rows(case.C, L + 5, in_off, stride_mod, torch).fill(x, L)  # 5 more floats of NaN in each row
    rref = ru.Rows(1, L + 5, ru.offsets(in_off, 3)[-1], 0, torch).fill(ref[None, :], L)
    wxx, vxx, mxx = double_rows(torch, case.C, K)
    wxy, vxy, mxy = double_rows(torch, case.C, 2 * K)
    wrr, vrr, mrr = double_rows(torch, 1, K)
    sp = d.api._welch_spec(case.H, case.window)
    ex = d.api._exec(rin.view, 0, None)
    import ctypes as C
    from dspbench import _lib as L_
    L_.check(L_.lib().dsp_welch(L_.chan_table(rin.ptrs()), case.C, L, C.cast(C.c_void_p(rref.ptrs()[0]), L_.FP),
                                d.api._dtable(vxx), d.api._dptr(vrr, 0), d.api._dtable(vxy), C.byref(sp), C.byref(ex)),
             "dsp_welch")
    torch.cuda.synchronize()
    got = (vxx.cpu().numpy(), vrr[0].cpu().numpy(), vxy.cpu().numpy())
    ru.assert_finite(*got)
    for whole, mask in ((wxx, mxx), (wxy, mxy), (wrr, mrr)):
        assert np.all(np.isnan(whole.cpu().numpy()[mask])), "an output guard was written"
    want = gpu_sums(x, ref, case.H, case.window)
    assert all(ru.same_bits(p, q) for p, q in zip(got, want))


def test_overlapping_rows_are_refused(torch_cuda):
    """An output row over an input row, over ref, or over another output row: DSP_ERR_INVALID, nothing written."""
    torch = torch_cuda
    L = 3 * wu.N
    buf = torch.zeros((2, L), dtype=torch.float32, device="cuda")
    buf[:] = 0.5
    ref = torch.full((L,), 0.25, dtype=torch.float32, device="cuda")
    ok = torch.full((2, 2 * K), 7.0, dtype=torch.float64, device="cuda")
    okx = torch.full((2, K), 7.0, dtype=torch.float64, device="cuda")
    okr = torch.full((K,), 7.0, dtype=torch.float64, device="cuda")
    over_in = buf.view(torch.float64)[:, :K]           # on the input rows
    over_ref = ref.view(torch.float64)[:K]             # on the reference
    same = okx[:1].expand(2, K)                        # two output rows in one place
    import ctypes as C
    from dspbench import _lib as L_

    def call(sxx, srr, sxy):
        sp, ex = d.api._welch_spec(4096, "hann"), d.api._exec(buf, 0, None)
        ptrs = [buf[c].data_ptr() for c in range(2)]
        return L_.lib().dsp_welch(L_.chan_table(ptrs), 2, L, C.cast(C.c_void_p(ref.data_ptr()), L_.FP),
                                  d.api._dtable(sxx), d.api._dptr(srr), d.api._dtable(sxy), C.byref(sp), C.byref(ex))

    for sxx, srr, sxy in ((over_in, okr, ok), (okx, over_ref, ok), (same, okr, ok), (okx, okx[1], ok),
                          (okx, okr, ok[:, K:].as_strided((2, 2 * K), (0, 1)))):
        assert call(sxx, srr, sxy) == L_.DSP_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.all(buf == 0.5) and torch.all(ref == 0.25)
    assert torch.all(ok == 7.0) and torch.all(okx == 7.0) and torch.all(okr == 7.0)
    assert call(okx, okr, ok) == L_.DSP_OK


def test_python_face_against_scipy(torch_cuda):
    """welch, csd and transfer on one small shape against scipy fed the same window;
    transfer against scipy's own H1 (so leakage bias cancels) within the coherence-implied
    random error |H| sqrt((1 - g) / (2 F g)) wherever the coherence g > 0.99."""
    import torch
    from scipy import signal
    sr, H, F = 48000.0, 2048, 31
    x, ref = wu.make_signals(wu.N + (F - 1) * H + 100, 2, seed=5)
    w = wm.window_table("hann").astype(np.float64)
    kw = dict(fs=sr, window=w, nperseg=wu.N, noverlap=wu.N - H, detrend=False)
    x64, r64 = x.astype(np.float64), ref.astype(np.float64)
    tx, tr = torch.from_numpy(x).cuda(), torch.from_numpy(ref).cuda()
    for scaling in ("density", "spectrum"):
        f, p = d.welch(tx, sr, H, "hann", scaling)
        fs, ps = signal.welch(x64, scaling=scaling, **kw)
        assert np.allclose(f, fs, rtol=1e-15, atol=0) and p.shape == ps.shape
        assert np.all(np.max(np.abs(p - ps), axis=1) <= wu.WELCH_TOL * ps.max(axis=1) * 2)  # (g <= 2 on the scale)
        f, pxy = d.csd(tr, tx, sr, H, "hann", scaling)
        cs = signal.csd(r64[None, :], x64, scaling=scaling, **kw)[1]
        prr = signal.welch(r64, scaling=scaling, **kw)[1]
        assert np.all(np.max(np.abs(pxy - cs), axis=1) <= wu.WELCH_TOL * 2 * np.sqrt(ps.max(axis=1) * prr.max()))
    f, H1, coh = d.transfer(tr, tx, sr, H, "hann")
    Hs = signal.csd(r64[None, :], x64, **kw)[1] / signal.welch(r64, **kw)[1]
    cohs = signal.coherence(r64[None, :], x64, **kw)[1]
    assert np.all(coh > 0.0) and np.all(coh < 1.0) and np.max(np.abs(coh - cohs)) <= 1e-4
    good = coh > 0.99
    assert good.sum() > 100
    err = np.abs(Hs) * np.sqrt((1.0 - coh) / (2 * F * coh))
    assert np.all(np.abs(H1 - Hs)[good] <= err[good])
