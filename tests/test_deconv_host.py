"""The host half of dsp_rfft / dsp_deconvolve / dsp_sweep (host_tables.cpp,
sweep_host.cpp through the C ABI): plans, the sweep against the float64 model of
tests/deconvutil.py, every refusal, the ctypes layouts, the no-device answer,
and the host code under ASan + UBSan from a stand-alone program.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L
import deconvutil as du

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "dsp-bench_amd")


def status_of(fn):
    with pytest.raises(d.DspError) as e:
        fn()
    return e.value.status


@pytest.mark.parametrize("Ly,Ls,n", [(1, 1, 1024), (1023, 1, 1024), (1024, 1024, 1024), (1025, 1, 2048), (1, 1025, 2048),
                                     (2 ** 14 - 1, 5, 2 ** 14), (2 ** 14, 2 ** 14, 2 ** 14), (2 ** 14 + 1, 9, 2 ** 15),
                                     (9, 2 ** 14 + 1, 2 ** 15), (2 ** 24, 1, 2 ** 24), (1, 2 ** 24, 2 ** 24)])
def test_deconv_plan(Ly, Ls, n):
    for C_ in (1, 2, 16, 17, 40):
        p = d.deconv_plan(Ly, Ls, C_)
        assert p["n"] == n == du.deconv_n(Ly, Ls)
        assert p["scratch_bytes"] == du.deconv_scratch_bytes(n, C_)


def test_deconv_plan_refusals():
    assert status_of(lambda: d.deconv_plan(2 ** 24 + 1, 1)) == -3
    assert status_of(lambda: d.deconv_plan(1, 2 ** 24 + 1)) == -3
    assert status_of(lambda: d.deconv_plan(0, 5)) == -1
    assert status_of(lambda: d.deconv_plan(5, 0)) == -1
    assert status_of(lambda: d.deconv_plan(5, 5, 0)) == -1


@pytest.mark.parametrize("b", range(10, 25))
def test_rfft_plan(b):
    n = 1 << b
    p = d.rfft_plan(n)
    assert p["radix"] == du.rfft_plan(n) and p["passes"] == len(p["radix"]) and 2 <= p["passes"] <= 4
    assert int(np.prod(p["radix"])) == n // 2 and set(p["radix"]) <= {64, 32, 8}
    assert p["scratch_bytes_per_channel"] == du.rfft_scratch_bytes(n) == 8 * n


@pytest.mark.parametrize("n", [0, 1, 512, 1023, 1025, 3 << 10, 2 ** 24 + 1, 2 ** 25])
def test_rfft_plan_refuses(n):
    assert status_of(lambda: d.rfft_plan(n)) == -1


SWEEPS = [dict(sr=48000, f1=20.0, f2=20000.0, seconds=1.0, amplitude=1.0, fade=0),
          dict(sr=48000, f1=50.0, f2=24000.0, seconds=0.25, amplitude=0.5, fade=6000),
          dict(sr=44100, f1=30.0, f2=15000.0, seconds=0.3337, amplitude=-0.8, fade=441),
          dict(sr=96000, f1=1.0, f2=2.0, seconds=0.001, amplitude=2.0, fade=48),
          du.SWEEP]


@pytest.mark.parametrize("s", SWEEPS, ids=lambda s: f"{s['sr']}-{s['seconds']}")
def test_sweep_matches_the_formula(s):
    x = d.sweep(**s)
    want = du.sweep64(**s)
    p = d.sweep_plan(**s)
    assert x.dtype == np.float32 and x.size == p["L"] == du.sweep_len(s["sr"], s["seconds"]) == int(round(s["seconds"] * s["sr"]))
    assert p["rate"] == pytest.approx(np.log(s["f2"] / s["f1"]) / s["seconds"], rel=1e-15)
    # libm and numpy may differ in the last double bit: within one float ulp of the rounded float64
    w32 = want.astype(np.float32)
    assert np.all(np.abs(x.astype(np.float64) - w32) <= np.spacing(np.abs(w32)))
    assert np.max(np.abs(x)) <= abs(s["amplitude"])


def test_sweep_fades():
    s = dict(sr=48000, f1=100.0, f2=10000.0, seconds=0.1, amplitude=1.0)
    plain, faded = d.sweep(**s, fade=0), d.sweep(**s, fade=480)
    w = 0.5 - 0.5 * np.cos(np.pi * (np.arange(480) + 0.5) / 480)
    assert np.allclose(faded[:480], plain[:480] * w, atol=1e-7) and np.allclose(faded[-480:], plain[-480:] * w[::-1], atol=1e-7)
    assert np.array_equal(faded[480:-480], plain[480:-480])
    whole = d.sweep(**s, fade=2400)  # 2 fade = L: allowed
    assert whole.size == 4800 and abs(whole[0]) < 1e-3


@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_harmonic_offset(order):
    got = d.sweep_harmonic_offset(48000, 50.0, 20000.0, 0.5, order)
    assert got == pytest.approx(du.harmonic_offset(48000, 50.0, 20000.0, 0.5, order), rel=1e-14)
    assert (got == 0.0) == (order == 1)


@pytest.mark.parametrize("bad", [dict(f1=0.0), dict(f1=-1.0), dict(f1=1000.0, f2=1000.0), dict(f1=2000.0, f2=1000.0),
                                 dict(f2=24001.0), dict(f1=float("nan")), dict(f2=float("nan")), dict(seconds=0.0),
                                 dict(seconds=-1.0), dict(seconds=float("nan")), dict(seconds=float("inf")),
                                 dict(seconds=350.0), dict(amplitude=float("inf")), dict(amplitude=float("nan")),
                                 dict(fade=24001), dict(seconds=1e-6), dict(sr=0)])
def test_sweep_refusals(bad):
    s = dict(dict(sr=48000, f1=20.0, f2=1000.0, seconds=1.0, amplitude=1.0, fade=0), **bad)
    assert status_of(lambda: d.sweep_plan(**s)) == -1
    assert status_of(lambda: d.sweep(**s)) == -1
    h = dict(s)
    del h["amplitude"], h["fade"]
    if not ({"amplitude", "fade"} & set(bad)):
        assert status_of(lambda: d.sweep_harmonic_offset(order=2, **h)) == -1


def test_sweep_refuses_count_and_order():
    sp = L.dsp_sweep_spec(20.0, 1000.0, 0.01, 1.0, 0)
    x = np.zeros(481, np.float32)
    lib = L.lib()
    assert lib.dsp_sweep(48000, C.byref(sp), d.api._fp(x), 481) == -1  # count > L
    assert lib.dsp_sweep(48000, C.byref(sp), d.api._fp(x), 480) == 0 and x[480] == 0.0
    assert lib.dsp_sweep(48000, None, d.api._fp(x), 1) == -1 and lib.dsp_sweep(48000, C.byref(sp), None, 1) == -1
    v = C.c_double()
    assert lib.dsp_sweep_harmonic_offset(48000, C.byref(sp), 0, C.byref(v)) == -1
    assert lib.dsp_sweep_plan(48000, C.byref(sp), None, None) == 0


def rows(a):
    return L.chan_table([a[c].ctypes.data for c in range(a.shape[0])]) if a is not None else None


def host_ex(offset=0):
    return L.dsp_exec(-1, L.DSP_EXEC_HOST_BUFFERS | L.DSP_EXEC_SYNC, None, offset)


def call_rfft(x, L_, n, spec, offset=0):
    ex = host_ex(offset)
    return L.lib().dsp_rfft(rows(x), x.shape[0], L_, n, rows(spec), C.byref(ex))


def call_irfft(spec, n, out, Lout, offset=0):
    ex = host_ex(offset)
    return L.lib().dsp_irfft(rows(spec), spec.shape[0], n, rows(out), Lout, C.byref(ex))


def call_deconv(rec, ref, ir, ir_len, sp=None, offset=0, Ly=None, Ls=None):
    ex = host_ex(offset)
    return L.lib().dsp_deconvolve(rows(rec), rec.shape[0], rec.shape[1] if Ly is None else Ly,
                                  d.api._fp(ref) if ref is not None else None, (ref.size if ref is not None else 5) if Ls is None else Ls,
                                  rows(ir), ir_len, C.byref(sp) if sp is not None else None, C.byref(ex))


def test_calls_refuse_bad_arguments_before_they_need_a_device():
    x, spec = np.zeros((2, 1024), np.float32), np.zeros((2, 1026), np.float32)
    assert call_rfft(x, 1024, 1000, spec) == -1 and call_rfft(x, 1024, 512, spec) == -1  # n
    assert call_rfft(x, 1025, 1024, spec) == -1  # L > n
    assert call_rfft(x, 1024, 1024, spec, offset=512) == -1
    buf = np.zeros((1, 4096), np.float32)
    assert call_rfft(buf[:, :1024], 1024, 1024, buf[:, 512:1538]) == -1  # the spectrum over its input
    assert call_rfft(x, 1024, 1024, np.lib.stride_tricks.as_strided(spec, (2, 1026), (8, 4))) == -1  # spectra overlap
    null_row = (L.FP * 2)()
    ex = host_ex()
    assert L.lib().dsp_rfft(rows(x), 2, 1024, 1024, null_row, C.byref(ex)) == -1
    assert L.lib().dsp_rfft(null_row, 2, 1024, 1024, rows(spec), C.byref(ex)) == -1
    out = np.zeros((2, 1024), np.float32)
    assert call_irfft(spec, 1000, out, 1024) == -1 and call_irfft(spec, 1024, out, 1025) == -1
    assert call_irfft(spec, 1024, out, 1024, offset=4) == -1
    assert call_irfft(spec, 1024, spec[:, 2:], 1024) == -1  # out over the spectrum
    assert L.lib().dsp_irfft(null_row, 2, 1024, rows(out), 1024, C.byref(ex)) == -1

    rec, ref, ir = np.ones((2, 1500), np.float32), np.ones(1200, np.float32), np.zeros((2, 2048), np.float32)
    sp = L.dsp_deconv_spec
    for eps in (0.0, 1e-13, 1.5, -1e-6, float("nan"), float("inf")):
        assert call_deconv(rec, ref, ir, 2048, sp(eps, 0)) == -1
    assert call_deconv(rec, ref, ir, 2049) == -1  # ir_len > n
    assert call_deconv(rec, ref, ir, 100, sp(1e-6, 101)) == -1  # pre > ir_len
    assert call_deconv(rec, ref, ir, 2048, offset=1) == -1
    assert call_deconv(rec, ref, ir, 2048, Ly=0) == -1 and call_deconv(rec, ref, ir, 2048, Ls=0) == -1
    assert call_deconv(rec[:0], ref, ir[:0], 2048) == -1  # C = 0
    assert call_deconv(rec, None, ir, 2048) == -1
    assert call_deconv(rec, ref, ir, 2048, Ly=2 ** 24 + 1) == -3
    assert call_deconv(rec, ref, rec[:, 100:], 1024) == -1  # ir over rec
    assert call_deconv(rec, ref, np.lib.stride_tricks.as_strided(ref, (2, 64), (0, 4)), 64) == -1  # ir over ref
    assert call_deconv(rec, ref, np.lib.stride_tricks.as_strided(ir, (2, 64), (8, 4)), 64) == -1  # ir rows overlap
    assert L.lib().dsp_deconvolve(rows(rec), 2, 1500, d.api._fp(ref), 1200, null_row, 64, None, C.byref(ex)) == -1


@pytest.mark.skipif(d.lib().dsp_device_count() > 0, reason="a GPU is visible")
def test_no_device_no_cpu_fallback():
    x, spec, out = np.ones((2, 1024), np.float32), np.zeros((2, 1026), np.float32), np.zeros((2, 1024), np.float32)
    assert call_rfft(x, 1024, 1024, spec) == -5 and not spec.any()
    assert call_irfft(spec, 1024, out, 1024) == -5 and not out.any()
    assert call_deconv(x, x[0].copy(), out, 1024) == -5 and not out.any()
    assert status_of(lambda: d.rfft(x, 1024)) == -5


def test_layout_and_exports():
    s, w = L.dsp_deconv_spec, L.dsp_sweep_spec
    assert C.sizeof(s) == 16 and [getattr(s, n).offset for n in ("eps", "pre")] == [0, 8]
    assert C.sizeof(w) == 40 and [getattr(w, n).offset for n in ("f1", "f2", "seconds", "amplitude", "fade")] == [0, 8, 16, 24, 32]
    lib = L.lib()
    for sym in ("dsp_rfft_plan", "dsp_rfft", "dsp_irfft", "dsp_deconv_plan", "dsp_deconvolve", "dsp_sweep_plan", "dsp_sweep",
                "dsp_sweep_harmonic_offset"):
        assert hasattr(lib, sym)
    for name in ("rfft", "irfft", "rfft_plan", "deconvolve", "deconv_plan", "sweep", "sweep_plan", "sweep_harmonic_offset"):
        assert callable(getattr(d, name)) and name in d.__all__
    assert lib.dsp_abi_version() == 3
    hdr = open(os.path.join(REPO, "include", "dspbench", "dspbench.h")).read()
    for text in ("double eps;", "uint32_t pre;", "double f1, f2, seconds, amplitude;", "uint32_t fade;",
                 "int dsp_rfft_plan(uint32_t n, uint32_t *passes, uint32_t radix[4], uint64_t *scratch_bytes_per_channel);"):
        assert text in hdr


def test_host_code_under_sanitizers(tmp_path):
    """tests/sanitize/deconv_host_check.cpp: a stand-alone program over the
    plans, the twiddle tables and the sweep at their corners, under ASan + UBSan."""
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
    exe = str(tmp_path / "deconv_host_check")
    cmd = [gxx, *flags, f"-I{REPO}/include", f"-I{PKG}/csrc", f"{HERE}/sanitize/deconv_host_check.cpp",
           f"{PKG}/csrc/sweep_host.cpp", f"{PKG}/csrc/host_tables.cpp", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "deconv host check ok" in r.stdout
