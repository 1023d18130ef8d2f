"""dsp_decay on the GPU (decay.hip and fft_big.hip's transforms) against the
float64 model of tools/decay_model.py (tests/decayutil.py: the cases, the
references, computed once, and DECAY_TOL), against itself, on unaligned,
strided and guarded rows, and end to end through dspbench.decay."""
import ctypes as C
import functools

import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L_
import decayutil as du
import decay_model as dm
import rowsutil as ru

pytestmark = pytest.mark.gpu


def gpu_energies(x, sr, bands, moments=True):
    """dsp_decay on device rows -> numpy (peak, onset, energy, moment)."""
    import torch
    tx = torch.from_numpy(np.array(x, np.float32)).cuda()  # (a copy: the cases are read-only)
    return tuple(None if a is None else a.cpu().numpy() for a in d.decay_energies(tx, sr, *bands, moments=moments))


@functools.lru_cache(maxsize=None)
def case_run(case):
    out = gpu_energies(du.make_case(case), case.sr, case.bands)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("case", du.CASES, ids=du.case_id)
def test_parity_with_float64(torch_cuda, case):
    """peak and onset equal the model's; per row max_j |e - e64| <= DECAY_TOL max_j e64, entry
    0 included; moments within the same bound times L."""
    peak, onset, e, m = case_run(case)
    wpeak, wonset, we, wm = du.reference(case)
    p = d.decay_plan(case.L, case.sr, *case.bands, case.C)
    assert e.shape == we.shape == (case.C, p["bands"], p["hops"]) and p["n"] <= 1 << 17
    assert ru.same_bits(peak, wpeak) and np.array_equal(onset.astype(np.uint64), wonset)
    assert np.all(wonset == du.expected_onset(case))
    ru.assert_finite(e, m)
    rm = np.max(np.max(np.abs(m - wm), axis=-1) / (case.L * we.max(axis=-1)))
    print(f"decay ratio {case.name} energy {dm.ratios(e, we):.3e} moment/L {rm:.3e}")
    du.check_energies(e, m, we, wm, case.L)
    npost = -(-(case.L - int(wonset[0])) // p["hop"])
    assert not e[:, :, 1 + npost:].any() and not m[:, :, 1 + npost:].any()


CASE_SMALL = du.CASES[9]  # C2-b10


def test_silence_gives_zeros(torch_cuda):
    peak, onset, e, m = gpu_energies(np.zeros((2, 3000), np.float32), 48000, du.OCT_HIGH)
    assert not peak.any() and not onset.any() and not e.any() and not m.any()
    assert np.all(np.signbit(e) == 0)


def test_two_calls_same_bits(torch_cuda):
    x = du.make_case(CASE_SMALL)
    a, b = gpu_energies(x, CASE_SMALL.sr, CASE_SMALL.bands), gpu_energies(x, CASE_SMALL.sr, CASE_SMALL.bands)
    assert all(ru.same_bits(p, q) for p, q in zip(a, b))
    assert all(ru.same_bits(p, q) for p, q in zip(a, case_run(CASE_SMALL)))


def test_bits_do_not_depend_on_C_or_band_count(torch_cuda):
    """Channel c, band b alone and among 17 channels and 32 bands: the same bits.  (n is the
    lowest band's: the lone call names a range that starts at the same band.)"""
    case = du.CASES[10]
    assert case.C == du.MAXCH + 1 and case.bands == du.THIRDS32
    x = du.make_case(case)
    peak, onset, e, m = case_run(case)
    f, k_lo, k_hi = case.bands
    for c in (0, du.MAXCH - 1, du.MAXCH):
        a = gpu_energies(x[c:c + 1], case.sr, (f, k_lo, k_lo))          # one channel, one band
        assert ru.same_bits(a[2][0, 0], e[c, 0]) and ru.same_bits(a[3][0, 0], m[c, 0])
        assert a[0][0] == peak[c] and a[1][0] == onset[c]
        a = gpu_energies(x[c:c + 1], case.sr, (f, k_lo, k_lo + 16))      # one channel, 17 bands: other groups
        assert ru.same_bits(a[2][0], e[c, :17]) and ru.same_bits(a[3][0], m[c, :17])
    a = gpu_energies(x[3:5], case.sr, case.bands, moments=False)
    assert a[3] is None and ru.same_bits(a[2], e[3:5])


def test_host_rows_same_bits(torch_cuda):
    x = np.ascontiguousarray(du.make_case(CASE_SMALL))
    dev = case_run(CASE_SMALL)
    host = d.decay_energies(x, CASE_SMALL.sr, *CASE_SMALL.bands)
    assert ru.same_bits(host[0], dev[0]) and np.array_equal(host[1].astype(np.int64), dev[1].astype(np.int64))
    assert ru.same_bits(host[2], dev[2]) and ru.same_bits(host[3], dev[3])


def double_rows(torch, R, n):
    """R float64 rows of n in one NaN-filled allocation with guards between them."""
    Gd = 16
    whole = torch.full((R * (n + Gd) + Gd,), float("nan"), dtype=torch.float64, device="cuda")
    view = whole.as_strided((R, n), (n + Gd, 1), Gd)
    mask = np.ones(whole.shape[0], bool)
    for r in range(R):
        mask[Gd + r * (n + Gd):Gd + r * (n + Gd) + n] = False
    return whole, view, mask


def raw_call(torch, ptrs, C_, L, sr, bands, peak, onset, ve, vm, ref):
    sp = L_.dsp_decay_spec(*bands)
    ex = d.api._exec(ref, 0, None)
    return L_.lib().dsp_decay(L_.chan_table(ptrs), C_, L, sr, C.byref(sp), C.cast(C.c_void_p(peak.data_ptr()), L_.FP),
                              C.cast(C.c_void_p(onset.data_ptr()), C.POINTER(C.c_uint64)), d.api._dtable(ve),
                              None if vm is None else d.api._dtable(vm), C.byref(ex))


@pytest.mark.parametrize("layout", ru.ALL)
def test_row_layouts(torch_cuda, layout):
    """Unaligned (4-byte) and strided input rows, NaN before and after every row: the aligned
    call's bits, nothing non-finite, and the output guards untouched."""
    torch = torch_cuda
    case = du.Case("layout", 1000 + 7 * 48 + 5, 48000, (1, 2, 3), 3, "noise", 100)
    x = du.make_signal(case, 11)
    in_off, _, stride_mod = ru.LAYOUTS[layout]
    rin = ru.Rows(case.C, case.L + 5, in_off, stride_mod, torch).fill(x, case.L)  # 5 more floats of NaN in each row
    p = d.decay_plan(case.L, case.sr, *case.bands, case.C)
    R = case.C * p["bands"]
    we, ve, me = double_rows(torch, R, p["hops"])
    wm_, vm, mm = double_rows(torch, R, p["hops"])
    peak = torch.full((case.C + 2,), float("nan"), dtype=torch.float32, device="cuda")
    onset = torch.full((case.C + 2,), -7, dtype=torch.int64, device="cuda")
    L_.check(raw_call(torch, rin.ptrs(), case.C, case.L, case.sr, case.bands, peak[1:], onset[1:], ve, vm, rin.view),
             "dsp_decay")
    torch.cuda.synchronize()
    got_e, got_m = ve.cpu().numpy(), vm.cpu().numpy()
    ru.assert_finite(got_e, got_m, peak[1:-1].cpu().numpy())
    for whole, mask in ((we, me), (wm_, mm)):
        assert np.all(np.isnan(whole.cpu().numpy()[mask])), "an output guard was written"
    assert torch.isnan(peak[0]) and torch.isnan(peak[-1]) and onset[0] == -7 and onset[-1] == -7
    want = gpu_energies(x, case.sr, case.bands)
    assert ru.same_bits(peak[1:-1].cpu().numpy(), want[0]) and np.array_equal(onset[1:-1].cpu().numpy(), want[1])
    assert ru.same_bits(got_e.reshape(want[2].shape), want[2]) and ru.same_bits(got_m.reshape(want[3].shape), want[3])


def test_overlap_and_misalignment_are_refused(torch_cuda):
    """An output row over an input row or another output row, a float64 row 4 bytes off,
    C = 0, L = 0 and a sample offset: DSP_ERR_INVALID, nothing written."""
    torch = torch_cuda
    L, sr, bands = 4000, 48000, (1, 2, 3)
    p = d.decay_plan(L, sr, *bands, 2)
    hops, R = p["hops"], 4
    buf = torch.full((2, L), 0.5, dtype=torch.float32, device="cuda")
    e = torch.full((R, hops), 7.0, dtype=torch.float64, device="cuda")
    m = torch.full((R, hops), 7.0, dtype=torch.float64, device="cuda")
    peak = torch.full((2,), 7.0, dtype=torch.float32, device="cuda")
    onset = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    ptrs = [buf[c].data_ptr() for c in range(2)]
    over_in = buf.view(torch.float64)[:1, :hops].expand(R, hops)
    same = e[:1].expand(R, hops)
    off4 = torch.full((R * (hops + 1) * 2,), 7.0, dtype=torch.float32, device="cuda")[1:].as_strided(
        (R, 2 * hops), (2 * hops + 2, 1))

    def call(ve, vm, pk=peak, on=onset, C_=2, L_n=L):
        return raw_call(torch, ptrs, C_, L_n, sr, bands, pk, on, ve, vm, buf)

    assert call(over_in, m) == L_.DSP_ERR_INVALID
    assert call(e, over_in) == L_.DSP_ERR_INVALID
    assert call(same, m) == L_.DSP_ERR_INVALID
    assert call(e, e) == L_.DSP_ERR_INVALID
    assert call(e, m, pk=buf[0]) == L_.DSP_ERR_INVALID
    assert call(e, m, on=e.view(torch.int64)[0]) == L_.DSP_ERR_INVALID

    class Off4:  # a table of row pointers 4 bytes past an 8-byte boundary
        shape = (R, hops)

        def __getitem__(self, r):
            return off4[r]
    assert off4[0].data_ptr() % 8 == 4 and call(Off4(), m) == L_.DSP_ERR_INVALID
    assert call(e, m, C_=0) == L_.DSP_ERR_INVALID and call(e, m, L_n=0) == L_.DSP_ERR_INVALID
    sp, ex = L_.dsp_decay_spec(*bands), d.api._exec(buf, 1, None)
    assert L_.lib().dsp_decay(L_.chan_table(ptrs), 2, L, sr, C.byref(sp), C.cast(C.c_void_p(peak.data_ptr()), L_.FP),
                              C.cast(C.c_void_p(onset.data_ptr()), C.POINTER(C.c_uint64)), d.api._dtable(e),
                              d.api._dtable(m), C.byref(ex)) == L_.DSP_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.all(buf == 0.5) and torch.all(e == 7.0) and torch.all(m == 7.0) and torch.all(off4 == 7.0)
    assert torch.all(peak == 7.0) and torch.all(onset == 7)
    assert call(e, m) == L_.DSP_OK


def test_end_to_end_decay_times(torch_cuda):
    """dspbench.decay on the decaying-sines impulse response: T20 and T30 within 1 % of the
    designed T and C50 within 0.1 dB of the float64 model (a sanity cap: the model alone
    stays within 0.2 %, test_decay_host.py)."""
    import torch
    case = du.CASES[11]
    assert case.name == "sines-48k"
    x = du.make_case(case)
    r = d.decay(torch.from_numpy(np.ascontiguousarray(x)).cuda(), case.sr, case.bands)
    _, onset, e, m = du.reference(case)
    assert r["onset"][0] == 38 and r["hop"] == 48 and r["t20"].shape == (1, 7)
    assert np.allclose(r["fm"], 1000.0 * dm.G ** np.arange(-3, 4))
    for b, T in ((0, 1.0), (3, 0.6), (6, 0.3)):
        want = dm.derive(e[0, b], m[0, b], case.L, 38, 48, case.sr)
        assert r["flags"][0, b] == 0
        assert abs(r["t20"][0, b] - T) <= 0.01 * T and abs(r["t30"][0, b] - T) <= 0.01 * T
        assert abs(r["c50"][0, b] - want["c50"]) <= 0.1
