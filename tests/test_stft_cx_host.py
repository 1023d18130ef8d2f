"""The host half of dsp_stft / dsp_istft (stft_cx_host.cpp through the C ABI):
both plans, every refusal that needs no device with dsp_last_error naming the
argument, the float64 models of tools/stft_model.py against torch on the CPU (the
convention), the float32 models against them on the GPU tests' shapes (the model
halves of STFT_TOL and ISTFT_TOL), the ABI version, and the host code under
ASan + UBSan from a stand-alone program.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L
import cstftutil as cu
import stft_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "dsp-bench_amd")
N, K = cu.N, cu.K


def refused(fn, status, *words):
    with pytest.raises(d.DspError) as e:
        fn()
    assert e.value.status == status, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@pytest.mark.parametrize("L_,H,F", [(8192, 4096, 1), (8191 + 4096, 4096, 1), (8192 + 4096, 4096, 2), (8192 + 99, 1, 100),
                                    (3 * 8192 - 1, 8192, 2), (48000 * 3600, 4096, 42186), (8192 + 4095 * 7, 4095, 8),
                                    (8192 + 512 * 9 + 511, 512, 10), (8192 + 513 * 9, 513, 10)])
def test_forward_plan(L_, H, F):
    for C_ in (1, 2, 17, 40):
        p = d.stft_plan(L_, C_, H)
        assert p == {"frames": F, "bins": 4097, "min_ld": 8194}
        assert F == sm.frame_count(L_, H) == d.stft_frames(L_, 8192, H)


@pytest.mark.parametrize("H,overlap", [(512, 16), (513, 16), (1024, 8), (2730, 4), (4095, 3), (4096, 2), (8191, 2), (8192, 1)])
def test_inverse_plan(H, overlap):
    for C_, rows, chunk in ((1, 1, 2048), (2, 2, 1024), (3, 3, 682), (16, 16, 128), (17, 16, 128), (100, 16, 128)):
        for F in (1, 2, overlap, chunk - 1, chunk, chunk + 1, 10 * chunk + 7, 48000 * 3600 // H):
            p = d.istft_plan(F, C_, H)
            assert p["Lout"] == N + (F - 1) * H == sm.full_length(F, H)
            assert p["overlap"] == overlap == -(-N // H) and p["chunk"] == chunk == (64 << 20) // (rows * 32768)
            assert p["scratch_bytes"] == rows * min(F, chunk + overlap - 1) * 32768 <= 72 << 20
    # the plan is the forward one's inverse
    assert d.stft_plan(d.istft_plan(9, 1, H)["Lout"], 1, H)["frames"] == 9


def test_plan_refusals():
    I, U = L.DSP_ERR_INVALID, L.DSP_ERR_UNSUPPORTED
    refused(lambda: d.stft_plan(8191), I, "L < N")
    refused(lambda: d.stft_plan(0), I, "L < N")
    refused(lambda: d.stft_plan(10 ** 5, 0), I, "C")
    refused(lambda: d.stft_plan(10 ** 5, hop=0), I, "H")
    refused(lambda: d.stft_plan(10 ** 5, hop=8193), I, "H")
    refused(lambda: d.stft_plan(10 ** 5, window=L.DSP_WIN_RECT), I, "window")
    refused(lambda: d.stft_plan(10 ** 5, window=7), I, "window")
    for n in (4096, 16384, 0, 8191):
        refused(lambda: d.stft_plan(10 ** 5, N=n), U, "N")
        refused(lambda: d.istft_plan(5, N=n), U, "N")
    assert d.stft_plan(10 ** 5, hop=8192)["frames"] == 12 and d.stft_plan(10 ** 5, hop=1)["frames"] == 10 ** 5 - 8191
    refused(lambda: d.istft_plan(0), I, "F")
    refused(lambda: d.istft_plan(5, 0), I, "C")
    refused(lambda: d.istft_plan(5, hop=0), I, "H")
    refused(lambda: d.istft_plan(5, hop=8193), I, "H")
    for h in (1, 256, 511):  # only the forward direction takes a small hop
        refused(lambda: d.istft_plan(5, hop=h), U, "H")
        assert d.stft_plan(10 ** 5, hop=h)["frames"] > 0
    refused(lambda: d.istft_plan(5, window=L.DSP_WIN_RECT), I, "window")
    for fl in (0.0, 9.9e-13, 1.0000001, -1e-10, float("inf"), float("nan")):
        refused(lambda: d.istft_plan(5, floor=fl), I, "floor")
    assert d.istft_plan(5, floor=1e-12)["Lout"] == d.istft_plan(5, floor=1.0)["Lout"] == N + 4 * 4096
    refused(lambda: d.istft_plan(2 ** 63), U, "Lout")
    # NULL specs: N 8192, H 4096, Hann, floor 1e-10
    f, lo, ov = C.c_uint64(), C.c_uint64(), C.c_uint32()
    assert L.lib().dsp_stft_plan(8192 * 3, 1, None, C.byref(f), None, None) == 0 and f.value == 5
    assert L.lib().dsp_istft_plan(5, 1, None, C.byref(lo), C.byref(ov), None, None) == 0
    assert lo.value == 8192 * 3 and ov.value == 2


def test_call_refusals_need_no_device():
    """Every argument error is reported before a device is looked for, and nothing is written."""
    F, n = 3, 8192 * 2
    x = np.full((2, n), 0.5, np.float32)
    Z = np.full((2, F, K), 7.0, np.complex64)
    y = np.full((2, n), 3.0, np.float32)
    lib = L.lib()
    rows = lambda a, off=0: L.chan_table([a[c].ctypes.data + off for c in range(a.shape[0])])  # noqa: E731
    ex = L.dsp_exec(-1, L.DSP_EXEC_HOST_BUFFERS | L.DSP_EXEC_SYNC, None, 0)
    off_ex = L.dsp_exec(-1, L.DSP_EXEC_HOST_BUFFERS, None, 4096)
    I, U = L.DSP_ERR_INVALID, L.DSP_ERR_UNSUPPORTED

    def fwd(in_=None, C_=2, n_=n, spec=None, ld=2 * K, sp=None, ex_=ex):
        return lib.dsp_stft(rows(x) if in_ is None else in_, C_, n_, rows(Z) if spec is None else spec, ld, sp,
                            C.byref(ex_))

    def inv(spec=None, C_=2, F_=F, ld=2 * K, out=None, Lout=n, sp=None, ex_=ex):
        return lib.dsp_istft(rows(Z) if spec is None else spec, C_, F_, ld, rows(y) if out is None else out, Lout, sp,
                             C.byref(ex_))

    def err():
        return lib.dsp_last_error().decode()

    S, IS = L.dsp_stft_spec, L.dsp_istft_spec
    for call, status, word in (
            (lambda: fwd(C_=0), I, "C"), (lambda: fwd(n_=8191), I, "L < N"),
            (lambda: fwd(sp=C.byref(S(8192, 0, 1))), I, "H"), (lambda: fwd(sp=C.byref(S(8192, 8193, 1))), I, "H"),
            (lambda: fwd(sp=C.byref(S(8192, 4096, 2))), I, "window"), (lambda: fwd(sp=C.byref(S(4096, 2048, 1))), U, "N"),
            (lambda: fwd(ld=2 * K + 1), I, "ld"), (lambda: fwd(ld=2 * K - 2), I, "ld"), (lambda: fwd(ld=0), I, "ld"),
            (lambda: fwd(ex_=off_ex), I, "sample_offset"),
            (lambda: fwd(in_=L.chan_table([0, 0])), I, "in"), (lambda: fwd(spec=L.chan_table([0, 0])), I, "spec"),
            (lambda: fwd(spec=rows(Z, 4)), I, "aligned"),
            (lambda: fwd(spec=L.chan_table([Z[0].ctypes.data] * 2)), I, "overlaps"),
            (lambda: fwd(spec=L.chan_table([x[0].ctypes.data, Z[1].ctypes.data]), n_=8192), I, "overlaps"),
            (lambda: inv(C_=0), I, "C"), (lambda: inv(F_=0), I, "F"),
            (lambda: inv(sp=C.byref(IS(8192, 0, 1, 1e-10))), I, "H"), (lambda: inv(sp=C.byref(IS(8192, 8193, 1, 1e-10))), I, "H"),
            (lambda: inv(sp=C.byref(IS(8192, 511, 1, 1e-10))), U, "H"),
            (lambda: inv(sp=C.byref(IS(8192, 4096, 2, 1e-10))), I, "window"),
            (lambda: inv(sp=C.byref(IS(8192, 4096, 1, 2.0))), I, "floor"),
            (lambda: inv(sp=C.byref(IS(8192, 4096, 1, float("nan")))), I, "floor"),
            (lambda: inv(sp=C.byref(IS(4096, 2048, 1, 1e-10))), U, "N"),
            (lambda: inv(ld=2 * K + 1), I, "ld"), (lambda: inv(ld=2 * K - 2), I, "ld"),
            (lambda: inv(Lout=0), I, "Lout"), (lambda: inv(Lout=N + (F - 1) * 4096 + 1), I, "Lout"),
            (lambda: inv(ex_=off_ex), I, "sample_offset"),
            (lambda: inv(spec=rows(Z, 4)), I, "aligned"), (lambda: inv(out=L.chan_table([0, 0])), I, "out"),
            (lambda: inv(out=L.chan_table([y[0].ctypes.data] * 2)), I, "overlaps"),
            (lambda: inv(out=L.chan_table([y[0].ctypes.data, Z[1].ctypes.data + 64])), I, "overlaps")):
        assert call() == status
        assert word in err(), (word, err())
    assert np.all(x == 0.5) and np.all(Z == 7.0) and np.all(y == 3.0)
    # what is left is a valid call: no device here, or a run
    assert fwd() in (L.DSP_ERR_NO_DEVICE, L.DSP_OK) and inv() in (L.DSP_ERR_NO_DEVICE, L.DSP_OK)


def test_abi_version_is_still_3():
    assert L.lib().dsp_abi_version() == 3 == L.ABI_VERSION
    for name in ("dsp_stft_plan", "dsp_stft", "dsp_istft_plan", "dsp_istft"):
        assert hasattr(L.lib(), name)
    s, i = L.dsp_stft_spec, L.dsp_istft_spec
    assert C.sizeof(s) == 12 and C.sizeof(i) == 24 and i.floor.offset == 16
    hdr = open(os.path.join(REPO, "include", "dspbench", "dspbench.h")).read()
    assert "#define DSPBENCH_ABI_VERSION 3" in hdr and "} dsp_istft_spec;" in hdr


# ---------------------------------------------------------------------------
# the models: the convention against torch, float32 against float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,window", [(4096, "hann"), (2730, "hamming"), (513, "hamming")])
def test_float64_models_against_torch(H, window):
    """stft64 is torch.stft(center=False) in float64, transposed; istft64(stft64(x)) is x
    wherever den >= floor; with Hamming it is torch.istft(center=False) too (Hann's zero
    end fails torch's own envelope check, which is why floor exists)."""
    import torch
    F = 6
    x = np.random.default_rng(3).standard_normal((2, N + (F - 1) * H + 17)).astype(np.float32)
    w = torch.from_numpy(sm.window_table(window).astype(np.float64))
    X = sm.stft64(x, H, window)
    T = torch.stft(torch.from_numpy(x.astype(np.float64)), N, H, window=w, center=False, return_complex=True)
    assert X.shape == (2, F, K) and np.max(np.abs(X - T.transpose(1, 2).numpy())) <= 1e-11 * np.max(np.abs(X))
    y = sm.istft64(X, H, window)
    den, _ = sm.envelope(F, H, window)
    ok = den >= cu.FLOOR
    assert y.shape == (2, sm.full_length(F, H)) and np.all(y[:, ~ok] == 0)
    assert np.max(np.abs(y - x[:, :y.shape[1]])[:, ok]) <= 1e-9  # (den down to 1e-10 amplifies 1e-16 rounding)
    if window == "hamming":
        assert ok.all()
        t = torch.istft(T, N, H, window=w, center=False).numpy()
        assert t.shape == y.shape and np.max(np.abs(t - y)) <= 1e-12
    else:
        assert not ok.all()
        with pytest.raises(RuntimeError):
            torch.istft(T, N, H, window=w, center=False)


def test_envelope():
    """den and the noise gain over the float table: 1 / w under one frame, and the classes of the default floor."""
    w = sm.window_table("hamming").astype(np.float64)
    den, A = sm.envelope(1, 4096, "hamming")
    assert np.allclose(den, w * w, rtol=1e-15) and np.allclose(A, 1 / w, rtol=1e-14)
    den, A = sm.envelope(3, 4096, "hann")
    assert den[0] == 0 and A[0] == 0 and den.size == N + 2 * 4096 and np.all(A[den > 0] >= 1 - 1e-12)
    for c in cu.INVERSE:
        e = cu.envelope(c.F, c.H, c.window)
        assert e.hi.sum() + e.lo.sum() + e.band.sum() == e.den.size
        assert (c.window == "hann") == bool(e.lo.any())


@pytest.mark.parametrize("case", cu.FORWARD, ids=cu.case_id)
def test_float32_forward_model_against_float64(case):
    """The model half of STFT_TOL on exactly the GPU tests' shapes: each case within MODEL_RATIO_FWD."""
    r = sm.ratios(sm.stft32(cu.make_input(case), case.H, case.window), cu.forward_reference(case))
    assert r <= cu.MODEL_RATIO_FWD * 1.001 and cu.MODEL_RATIO_FWD <= cu.STFT_TOL / 4


@pytest.mark.parametrize("case", cu.INVERSE, ids=cu.case_id)
def test_float32_inverse_model_against_float64(case):
    Z, ref = cu.make_spectrum(case), cu.inverse_reference(case)
    r = cu.inverse_ratio(sm.istft32(Z, case.H, case.window), ref.q, cu.envelope(case.F, case.H, case.window), ref.vmax)
    assert r <= cu.MODEL_RATIO_INV * 1.001 and cu.MODEL_RATIO_INV <= cu.ISTFT_TOL / 4


def test_tolerances_are_four_times_the_worst_ratio():
    assert cu.STFT_TOL == 4 * max(cu.MODEL_RATIO_FWD, cu.GPU_RATIO_FWD)
    assert cu.ISTFT_TOL == 4 * max(cu.MODEL_RATIO_INV, cu.GPU_RATIO_INV)
    # the same packed FFT meets 1e-6 of the frame's peak in dsp_stft_magnitude
    assert cu.GPU_RATIO_FWD <= 1e-6 and cu.GPU_RATIO_INV <= 1e-6
    assert len(cu.FORWARD) == 32 and len(cu.INVERSE) == 21 and all(c.H >= 512 for c in cu.INVERSE)


def test_host_code_under_sanitizers(tmp_path):
    """tests/sanitize/stft_cx_host_check.cpp: a stand-alone program over both plans and the
    chunk walk at the extremes (L and F near 2^63, H = 1, C = 2^32 - 1), under ASan + UBSan."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # whether the compiler has the sanitizers' runtime: a trivial program, so that
    # an error in the check program itself fails below instead of skipping
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([gxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True,
                       timeout=300)
    if r.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "stft_cx_host_check")
    cmd = [gxx, *flags, f"-I{REPO}/include", f"-I{PKG}/csrc", f"{HERE}/sanitize/stft_cx_host_check.cpp",
           f"{PKG}/csrc/stft_cx_host.cpp", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "stft_cx host check ok" in r.stdout
