"""The host half of dsp_welch (welch_host.cpp through the C ABI): the plan, every
refusal that needs no device, dsp_welch_derive against scipy fed float64 sums,
the float32 model of tools/welch_model.py against float64 on the GPU tests'
shapes (the model half of WELCH_TOL), and the ABI version.  No GPU."""
import ctypes as C

import numpy as np
import pytest
from scipy import signal

import dspbench as d
from dspbench import _lib as L
import welchutil as wu
import welch_model as wm


def status_of(fn):
    with pytest.raises(d.DspError) as e:
        fn()
    return e.value.status


@pytest.mark.parametrize("L_,H,F", [(8192, 4096, 1), (8191 + 4096, 4096, 1), (8192 + 4096, 4096, 2), (8192 + 99, 1, 100),
                                    (3 * 8192 - 1, 8192, 2), (48000 * 3600, 4096, 42186), (8192 + 4095 * 7, 4095, 8)])
def test_plan_frames_bins_run(L_, H, F):
    for C_, has_ref in ((1, False), (2, True), (17, True), (40, False)):
        p = d.welch_plan(L_, C_, has_ref, H)
        assert p["frames"] == F == wm.frame_count(L_, H) == d.stft_frames(L_, 8192, H)
        assert p["bins"] == 4097 and p["run"] == wu.RUN == 16
        assert p["scratch_bytes"] == wu.scratch_bytes(F, C_, has_ref)


def test_plan_scratch_is_bounded():
    """Above the cap the scratch does not depend on L; it never exceeds 72 MiB."""
    for C_, has_ref in ((1, False), (1, True), (2, True), (16, False), (17, True), (100, True)):
        big = [d.welch_plan(L_, C_, has_ref, H)["scratch_bytes"] for L_, H in
               ((48000 * 3600, 4096), (48000 * 36000, 4096), (2 ** 31 + 12345, 1), (10 ** 8, 8192))]
        assert len(set(big)) == 1 and big[0] <= 72 << 20
        small = d.welch_plan(8192 * 4, C_, has_ref)["scratch_bytes"]
        assert small < big[0]


@pytest.mark.parametrize("window", ["hann", "hamming"])
def test_plan_window_sums(window):
    w = wm.window_table(window).astype(np.float64)
    p = d.welch_plan(8192, 1, False, 4096, window)
    assert p["win_sum"] == pytest.approx(np.sum(w), rel=1e-12)
    assert p["win_sumsq"] == pytest.approx(np.sum(w * w), rel=1e-12)
    a, b = wm.WINDOWS[window]  # the symmetric convention, not scipy's periodic default
    assert p["win_sum"] == pytest.approx(np.sum(signal.get_window(window, 8192, fftbins=False)), rel=1e-7)
    assert w[0] == pytest.approx(a - b, abs=1e-7) and w[0] == w[-1]


def test_plan_refusals():
    assert status_of(lambda: d.welch_plan(8191)) == L.DSP_ERR_INVALID            # F = 0
    assert status_of(lambda: d.welch_plan(0)) == L.DSP_ERR_INVALID
    assert status_of(lambda: d.welch_plan(10 ** 5, 0)) == L.DSP_ERR_INVALID       # C = 0
    assert status_of(lambda: d.welch_plan(10 ** 5, hop=0)) == L.DSP_ERR_INVALID
    assert status_of(lambda: d.welch_plan(10 ** 5, hop=8193)) == L.DSP_ERR_INVALID
    assert status_of(lambda: d.welch_plan(10 ** 5, window=L.DSP_WIN_RECT)) == L.DSP_ERR_INVALID
    assert status_of(lambda: d.welch_plan(10 ** 5, window=7)) == L.DSP_ERR_INVALID
    for n in (4096, 16384, 0, 8191):
        assert status_of(lambda: d.welch_plan(10 ** 5, N=n)) == L.DSP_ERR_UNSUPPORTED
    assert d.welch_plan(10 ** 5, hop=8192)["frames"] == 12 and d.welch_plan(10 ** 5, hop=1)["frames"] == 10 ** 5 - 8191
    # a NULL spec: N 8192, H 4096, Hann
    f, ws = C.c_uint64(), C.c_double()
    assert L.lib().dsp_welch_plan(8192 * 3, 1, 0, None, C.byref(f), None, None, None, C.byref(ws), None) == 0
    assert f.value == 5 and ws.value == d.welch_plan(8192)["win_sum"]


def test_call_refusals_need_no_device():
    """Every argument error is reported before a device is looked for."""
    n = 8192 * 2
    x = np.zeros((2, n), np.float32)
    ref = np.zeros(n, np.float32)
    sxx, sxy, srr = np.zeros((2, 4097)), np.zeros((2, 2 * 4097)), np.zeros(4097)
    lib, t, p = L.lib(), d.api._dtable, d.api._dptr
    rows = L.chan_table([x[c].ctypes.data for c in range(2)])
    rp = C.cast(C.c_void_p(ref.ctypes.data), L.FP)
    ex = L.dsp_exec(-1, L.DSP_EXEC_HOST_BUFFERS | L.DSP_EXEC_SYNC, None, 0)

    def call(rows=rows, C_=2, n=n, ref=rp, sxx=t(sxx), srr=p(srr), sxy=t(sxy), spec=None, ex=ex):
        return lib.dsp_welch(rows, C_, n, ref, sxx, srr, sxy, spec, C.byref(ex))

    assert call(C_=0) == L.DSP_ERR_INVALID
    assert call(n=8191) == L.DSP_ERR_INVALID
    assert call(spec=C.byref(L.dsp_welch_spec(8192, 0, 1))) == L.DSP_ERR_INVALID
    assert call(spec=C.byref(L.dsp_welch_spec(8192, 8193, 1))) == L.DSP_ERR_INVALID
    assert call(spec=C.byref(L.dsp_welch_spec(8192, 4096, 2))) == L.DSP_ERR_INVALID
    assert call(spec=C.byref(L.dsp_welch_spec(4096, 2048, 1))) == L.DSP_ERR_UNSUPPORTED
    assert call(ex=L.dsp_exec(-1, L.DSP_EXEC_HOST_BUFFERS, None, 4096)) == L.DSP_ERR_INVALID
    # srr and sxy go with ref
    assert call(ref=None) == L.DSP_ERR_INVALID
    assert call(srr=None) == L.DSP_ERR_INVALID and call(sxy=None) == L.DSP_ERR_INVALID
    assert call(ref=None, srr=None) == L.DSP_ERR_INVALID
    assert call(sxx=None) == L.DSP_ERR_INVALID and call(rows=None) == L.DSP_ERR_INVALID
    # an output row 4 bytes off an 8-byte boundary
    raw = np.zeros(4097 * 8 + 16, np.uint8)
    off = (-raw.ctypes.data) % 8 + 4
    bad = C.cast(C.c_void_p(raw.ctypes.data + off), L.DP)
    assert call(srr=bad) == L.DSP_ERR_INVALID
    # overlaps: an output row on an input row, on ref, on another output row
    xin = C.cast(C.c_void_p(x[1].ctypes.data), L.DP)
    assert call(srr=xin) == L.DSP_ERR_INVALID
    assert call(srr=C.cast(C.c_void_p(ref.ctypes.data + 8), L.DP)) == L.DSP_ERR_INVALID
    assert call(srr=p(sxx, 1)) == L.DSP_ERR_INVALID
    assert call(srr=C.cast(C.c_void_p(sxy[0].ctypes.data + 8 * 4097), L.DP)) == L.DSP_ERR_INVALID
    same = (L.DP * 2)(p(sxx, 0), p(sxx, 0))
    assert call(sxx=same) == L.DSP_ERR_INVALID
    assert not sxx.any() and not sxy.any() and not srr.any() and not x.any()
    # what is left is a valid call: no device here, or a run of silence
    assert call() in (L.DSP_ERR_NO_DEVICE, L.DSP_OK)


def derive_case(C_=3, F=9, H=2730, window="hamming", seed=3):
    x, ref = wu.make_signals(wu.N + (F - 1) * H + 17, C_, seed=seed)
    sxx, srr, sxy = wm.sums64(x, ref, H, window)
    w = wm.window_table(window).astype(np.float64)
    kw = dict(window=w, nperseg=wu.N, noverlap=wu.N - H, detrend=False)
    p = d.welch_plan(x.shape[1], C_, True, H, window)
    return x.astype(np.float64), ref.astype(np.float64), sxx, srr, np.ascontiguousarray(sxy).view(np.float64), kw, p, F


@pytest.mark.parametrize("scaling", ["density", "spectrum"])
def test_derive_against_scipy(scaling):
    """psd (both scalings, the DC and Nyquist factors), H1 and coherence from float64 sums: scipy's to 1e-12."""
    x, ref, sxx, srr, sxy, kw, p, F = derive_case()
    sr = 44100.0
    out = d.welch_derive(sxx, srr, sxy, F, sr, p["win_sum"], p["win_sumsq"], scaling)
    f, ps = signal.welch(x, fs=sr, scaling=scaling, **kw)
    assert np.max(np.abs(out["psd"] - ps) / ps) <= 1e-12
    assert np.all(ps[:, 0] > 0) and np.all(ps[:, -1] > 0)  # the undoubled ends are compared too
    pr = signal.welch(ref, fs=sr, scaling=scaling, **kw)[1]
    cs = signal.csd(ref[None, :], x, fs=sr, scaling=scaling, **kw)[1]
    Hs = cs / pr
    assert np.max(np.abs(out["H1"] - Hs) / np.abs(Hs)) <= 1e-12
    coh = signal.coherence(ref[None, :], x, fs=sr, **kw)[1]
    assert np.max(np.abs(out["coherence"] - coh) / coh) <= 1e-12
    assert np.all(out["coherence"] > 0) and np.all(out["coherence"] < 1)


def test_derive_zero_denominators_and_null_outputs():
    _, _, sxx, srr, sxy, _, p, F = derive_case(C_=2, F=3)
    sxx, srr = sxx.copy(), srr.copy()
    srr[5] = 0.0
    sxx[1, 9] = 0.0
    out = d.welch_derive(sxx, srr, sxy, F, 48000.0, p["win_sum"], p["win_sumsq"])
    assert np.all(out["H1"][:, 5] == 0) and np.all(out["coherence"][:, 5] == 0)
    assert out["coherence"][1, 9] == 0 and out["coherence"][0, 9] > 0 and out["H1"][1, 9] != 0
    assert np.all(np.isfinite(out["psd"])) and np.all(np.isfinite(out["coherence"])) and np.all(np.isfinite(out["H1"]))
    # any output may be NULL; the cross outputs need srr and sxy
    only = d.welch_derive(sxx, None, None, F, 48000.0, p["win_sum"], p["win_sumsq"])
    assert set(only) == {"psd"} and np.array_equal(only["psd"], out["psd"])
    cross = d.welch_derive(sxx, srr, sxy, F, 48000.0, p["win_sum"], p["win_sumsq"], psd=False)
    assert set(cross) == {"H1", "coherence"} and np.array_equal(cross["H1"], out["H1"])
    lib, t = L.lib(), d.api._dtable
    h = np.zeros((2, 2 * 4097))
    assert lib.dsp_welch_derive(t(sxx), None, None, 2, 4097, F, 1.0, 1.0, 1.0, 0, None, t(h), None) == L.DSP_ERR_INVALID
    assert lib.dsp_welch_derive(t(sxx), None, None, 0, 4097, F, 1.0, 1.0, 1.0, 0, None, None, None) == L.DSP_ERR_INVALID
    assert lib.dsp_welch_derive(t(sxx), None, None, 2, 4097, 0, 1.0, 1.0, 1.0, 0, None, None, None) == L.DSP_ERR_INVALID
    assert lib.dsp_welch_derive(t(sxx), None, None, 2, 4097, F, 1.0, 1.0, 1.0, 2, None, None, None) == L.DSP_ERR_INVALID
    assert lib.dsp_welch_derive(t(sxx), None, None, 2, 4097, F, 0.0, 1.0, 1.0, 0, t(h), None, None) == L.DSP_ERR_INVALID
    assert lib.dsp_welch_derive(t(sxx), None, None, 2, 4097, F, 1.0, 1.0, 1.0, 0, None, None, None) == L.DSP_OK


@pytest.mark.parametrize("case", wu.CASES, ids=wu.case_id)
def test_float32_model_against_float64(case):
    """The model half of WELCH_TOL on exactly the GPU tests' shapes: its worst ratio is
    MODEL_RATIO (each case within it), a quarter of the tolerance at most."""
    x, ref = wu.make_case(case)
    r = wm.ratios(wm.sums32(x, ref, case.H, case.window), wu.reference(case))
    assert max(r.values()) <= wu.MODEL_RATIO * 1.001 <= wu.WELCH_TOL / 4
    assert wu.WELCH_TOL == 4 * max(wu.MODEL_RATIO, wu.GPU_RATIO) and wu.GPU_RATIO <= 4 * wu.MODEL_RATIO


def test_model_scipy_and_order():
    """scipy with the scaling undone is sums64; the run-then-float64 order is what sums32 does."""
    case = wu.CASES[4]
    x, ref = wu.make_case(case)
    for a, b in zip(wm.scipy64(x, ref, case.H, case.window), wu.reference(case)):
        assert np.max(np.abs(a - b)) <= 1e-11 * np.max(np.abs(b))
    one = wm.sums32(x, ref, case.H, case.window, run=1)[0]    # every frame straight into float64
    runs = wm.sums32(x, ref, case.H, case.window)[0]
    assert not np.array_equal(one, runs) and np.max(np.abs(one - runs)) <= wu.WELCH_TOL * runs.max()


def test_abi_version_is_still_3():
    assert L.lib().dsp_abi_version() == 3 == L.ABI_VERSION
    for name in ("dsp_welch_plan", "dsp_welch", "dsp_welch_derive"):
        assert hasattr(L.lib(), name)
