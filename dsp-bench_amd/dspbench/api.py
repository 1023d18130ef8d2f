"""Python host mirror of the DSP-Bench hot path over libdspbench.

Buffers are either torch CUDA tensors (device-resident: the fast path, the
call is enqueued on the tensor's current HIP stream) or numpy arrays (host
buffers: the library stages them through HBM and synchronises).  Every
computation happens in the HIP kernels of libdspbench; this module only
marshals pointers.

Interface mirror (reference odecaux/DSP-Bench):
  Plugin.gain_test / ir_test / static_gain / no_op  stock plugins with their
      Parameters / State blobs laid out as the plugin structs
      (build/gain_test.cpp:14-16, build/IR_test.cpp:14-17,
      test/static_gain_plugin.cpp:7-9)
  render_offline   render_audio pumped block by block (audio.cpp:13-175)
  render_loop      the same with the file looping (audio.cpp:100-132)
  stft_magnitude   windowing -> fft_forward -> pythagore_array per frame
  render_stft      both, fused
  ir_analysis      compute_IR + fft_perform_and_get_magnitude
                   (plugin.cpp:17-58, dsp.cpp:53-66)
  fft_forward / fft_reverse   dsp.cpp:74-132
"""
from __future__ import annotations

import ctypes as C
import struct
import threading
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L
from ._lib import check, chan_table, dsp_exec, dsp_plugin

IR_BUFFER_LENGTH = 2048  # ref hardcoded_values.h:27
MAX_FFT_ORDER = 13       # ref hardcoded_values.h:6


@dataclass
class Plugin:
    kind: int
    params: bytes = b""
    state: bytes = b""
    name: str = ""
    module: object = None
    exec_flags: int = 0  # DSP_EXEC_* bits every call with this plugin adds (per call, no global)
    _keep: list = field(default_factory=list, repr=False)

    @staticmethod
    def gain_test(gain: float = 0.2) -> "Plugin":
        return Plugin(L.DSP_PLUGIN_GAIN, struct.pack("<f", gain), b"", "gain_test")

    @staticmethod
    def ir_test(gain: float = 0.9, step: float = 0.002, every_frame: bool = False) -> "Plugin":
        """every_frame: the fused render + STFT computes every frame's FFT
        (DSP_EXEC_EVERY_FRAME) even where all frames are the same (H % B == 0)."""
        return Plugin(L.DSP_PLUGIN_IR_RAMP, struct.pack("<ff", gain, step), b"", "IR_test",
                      exec_flags=L.DSP_EXEC_EVERY_FRAME if every_frame else 0)

    @staticmethod
    def static_gain(gain: float = 0.1) -> "Plugin":
        return Plugin(L.DSP_PLUGIN_STATIC_GAIN, b"", struct.pack("<f", gain), "static_gain_plugin")

    @staticmethod
    def no_op() -> "Plugin":
        return Plugin(L.DSP_PLUGIN_NOOP, b"", b"", "no_op")

    @staticmethod
    def fir(taps, direct: bool = False) -> "Plugin":
        """Build-defined FIR (cfg 3b): y[n] = sum_k taps[k] x[n - k].  The
        render uses FFT overlap-save for T <= 1025 taps unless `direct`
        (DSP_EXEC_FIR_DIRECT on every call with this plugin)."""
        t = np.ascontiguousarray(np.asarray(taps, dtype=np.float32))
        return Plugin(L.DSP_PLUGIN_FIR, t.tobytes(), b"", f"fir{t.size}",
                      exec_flags=L.DSP_EXEC_FIR_DIRECT if direct else 0)

    @staticmethod
    def conv(taps) -> "Plugin":
        """Convolution with a long impulse response (DSP_PLUGIN_CONV): FIR's
        semantics, y[n] = sum_k taps[k] x[n - k], for 1..2^20 finite taps, by
        partitioned FFT overlap-save (conv_plan gives its sizes)."""
        t = np.ascontiguousarray(np.asarray(taps, dtype=np.float32).reshape(-1))
        return Plugin(L.DSP_PLUGIN_CONV, t.tobytes(), b"", f"conv{t.size}")

    @staticmethod
    def biquad(sections) -> "Plugin":
        """Build-defined cascade of 1..4 direct-form-I biquads (DSP_PLUGIN_BIQUAD):
        `sections` = rows (b0, b1, b2, a1, a2), each y = b0 x + b1 x1 + b2 x2 -
        a1 y1 - a2 y2 (plugins/biquad.cpp's section), zero initial state, the
        whole file; rendered block-parallel by a state scan (iir.hip)."""
        c = np.ascontiguousarray(np.asarray(sections, dtype=np.float32).reshape(-1, 5))
        return Plugin(L.DSP_PLUGIN_BIQUAD, c.tobytes(), b"", f"biquad{c.shape[0]}")

    @staticmethod
    def biquad_lowpass_coefficients(cutoff: float = 1000.0, q: float = 0.7071, sr: float = 48000.0):
        """The coefficients plugins/biquad.cpp's initialize_state computes
        (RBJ cookbook low-pass in double, rounded to float), as one section row."""
        import math
        w0 = 2.0 * 3.14159265358979323846 * float(np.float32(cutoff)) / float(np.float32(sr))
        alpha = math.sin(w0) / (2.0 * float(np.float32(q)))
        c = math.cos(w0)
        a0 = 1.0 + alpha
        b0 = np.float32((1.0 - c) / 2.0 / a0)
        return np.array([[b0, np.float32((1.0 - c) / a0), b0, np.float32(-2.0 * c / a0),
                          np.float32((1.0 - alpha) / a0)]], np.float32)

    def as_struct(self) -> dsp_plugin:
        p = C.create_string_buffer(self.params, max(1, len(self.params)))
        s = C.create_string_buffer(self.state, max(1, len(self.state)))
        self._keep = [p, s]
        mod = self.module.handle if self.module is not None else None
        return dsp_plugin(self.kind, len(self.params), C.cast(p, C.c_void_p) if self.params else None,
                          len(self.state), C.cast(s, C.c_void_p) if self.state else None, mod)


# --------------------------------------------------------------------------
# buffer plumbing
# --------------------------------------------------------------------------

def _is_torch(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _rows(x):
    """Row pointers of a [C, L] buffer (torch CUDA or numpy)."""
    if x is None:
        return [], None
    if _is_torch(x):
        assert x.dtype.itemsize == 4 and x.dim() == 2 and x.stride(1) == 1
        return [x[c].data_ptr() for c in range(x.shape[0])], x
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2 and x.strides[1] == 4
    return [x[c].ctypes.data for c in range(x.shape[0])], x


def _exec(ref, sample_offset: int = 0, stream=None, sync: bool = False) -> dsp_exec:
    if ref is not None and _is_torch(ref):
        import torch
        dev = ref.device.index if ref.device.index is not None else torch.cuda.current_device()
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return dsp_exec(dev, L.DSP_EXEC_SYNC if sync else 0, C.c_void_p(st), sample_offset)
    return dsp_exec(-1, L.DSP_EXEC_HOST_BUFFERS | L.DSP_EXEC_SYNC, None, sample_offset)


def _alloc_like(ref, shape):
    if ref is not None and _is_torch(ref):
        import torch
        return torch.empty(shape, dtype=torch.float32, device=ref.device)
    return np.empty(shape, dtype=np.float32)


def conv_plan(taps: int, L_: int, B: int, C_out: int) -> tuple[int, int, int]:
    """DSP_PLUGIN_CONV's plan for `taps` taps over a call of L_ samples in blocks
    of B on C_out channels (dsp_conv_plan, host only): (partitions, frames,
    scratch bytes of one channel group)."""
    p, f, b = C.c_uint32(), C.c_uint64(), C.c_uint64()
    check(L.lib().dsp_conv_plan(taps, L_, B, C_out, C.byref(p), C.byref(f), C.byref(b)), "dsp_conv_plan")
    return p.value, f.value, b.value


def _resample_spec(zeros, beta, rolloff):
    """The three quality fields as a dsp_resample_spec, or None (the library's
    defaults) when none is given; a field left out takes its default."""
    if zeros is None and beta is None and rolloff is None:
        return None
    return L.dsp_resample_spec(64 if zeros is None else zeros, 14.769656459379492 if beta is None else beta,
                               0.9475937167399596 if rolloff is None else rolloff)


def resample_plan(sr_in: int, sr_out: int, L_: int = 0, zeros=None, beta=None, rolloff=None) -> dict:
    """dsp_resample_plan (host only): up, down, taps per phase, Lout and the
    table's bytes of a conversion of L_ samples."""
    spec = _resample_spec(zeros, beta, rolloff)
    up, down, taps, lout, tb = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
    check(L.lib().dsp_resample_plan(sr_in, sr_out, L_, C.byref(spec) if spec is not None else None, C.byref(up),
                                    C.byref(down), C.byref(taps), C.byref(lout), C.byref(tb)), "dsp_resample_plan")
    return {"up": up.value, "down": down.value, "taps": taps.value, "Lout": lout.value, "table_bytes": tb.value}


def resample_taps(sr_in: int, sr_out: int, zeros=None, beta=None, rolloff=None):
    """dsp_resample_taps (host only): the conversion's table [up, taps] float32."""
    p = resample_plan(sr_in, sr_out, 0, zeros, beta, rolloff)
    spec = _resample_spec(zeros, beta, rolloff)
    t = np.empty((p["up"], p["taps"]), np.float32)
    check(L.lib().dsp_resample_taps(sr_in, sr_out, C.byref(spec) if spec is not None else None, _fp(t), t.size),
          "dsp_resample_taps")
    return t


def resample(x, sr_in: int, sr_out: int, zeros=None, beta=None, rolloff=None, stream=None, out=None):
    """Sample-rate conversion of x [C, L] (torch CUDA tensor, or numpy on the
    host) from sr_in to sr_out (dsp_resample).  Returns [C, Lout]."""
    in_ptrs, ref = _rows(x)
    L_ = int(x.shape[1])
    lout = resample_plan(sr_in, sr_out, L_, zeros, beta, rolloff)["Lout"]
    if out is None:
        out = _alloc_like(ref, (len(in_ptrs), max(lout, 1)))
    out_ptrs, _ = _rows(out)
    spec = _resample_spec(zeros, beta, rolloff)
    ex = _exec(ref, 0, stream)
    check(L.lib().dsp_resample(chan_table(in_ptrs), len(in_ptrs), L_, chan_table(out_ptrs), lout, sr_in, sr_out,
                               C.byref(spec) if spec is not None else None, C.byref(ex)), "dsp_resample")
    return out[:, :lout]


def loudness_plan(sr: int, L_: int = 0) -> dict:
    """dsp_loudness_plan (host only): hop, hops, oversample and the device
    scratch bytes of a measurement of L_ samples at rate sr."""
    hop, hops, ovs, sb = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint64()
    check(L.lib().dsp_loudness_plan(sr, L_, C.byref(hop), C.byref(hops), C.byref(ovs), None, C.byref(sb)),
          "dsp_loudness_plan")
    return {"hop": hop.value, "hops": hops.value, "oversample": ovs.value, "scratch_bytes": sb.value}


def k_weighting(sr: int):
    """The K-weighting cascade at rate sr: float32 [2, 5], rows b0 b1 b2 a1 a2."""
    k = np.empty((2, 5), np.float32)
    check(L.lib().dsp_loudness_plan(sr, 0, None, None, None, _fp(k), None), "dsp_loudness_plan")
    return k


def _double_rows(a):
    t = (C.POINTER(C.c_double) * max(1, a.shape[0]))()
    for c in range(a.shape[0]):
        t[c] = C.cast(C.c_void_p(a[c].ctypes.data), C.POINTER(C.c_double))
    return t


def _weights(weights, channels):
    if weights is None:
        return None, None
    w = np.ascontiguousarray(weights, np.float32)
    assert w.shape == (channels,)
    return w, _fp(w)


_LOUDNESS_FIELDS = ("integrated", "range", "momentary_max", "short_term_max", "sample_peak", "true_peak")


def _loudness_dict(res, fields):
    out = {k: float(getattr(res, k)) for k in fields}
    out["blocks"], out["gated_blocks"] = int(res.blocks), int(res.gated_blocks)
    return out


def loudness_gate(hop_energy, hop: int, weights=None) -> dict:
    """dsp_loudness_gate (host only): integrated, range, momentary_max,
    short_term_max, blocks and gated_blocks from hop energies [C, hops]."""
    z = np.ascontiguousarray(hop_energy, np.float64)
    assert z.ndim == 2
    w, wp = _weights(weights, z.shape[0])
    res = L.dsp_loudness_result()
    check(L.lib().dsp_loudness_gate(_double_rows(z), z.shape[0], z.shape[1], hop, wp, C.byref(res)),
          "dsp_loudness_gate")
    return _loudness_dict(res, _LOUDNESS_FIELDS[:4])


def loudness(x, sr: int, weights=None, true_peak: bool = True, zeros=None, beta=None, rolloff=None,
             stream=None) -> dict:
    """Programme loudness of x [C, L] (torch CUDA tensor, or numpy on the host)
    at rate sr (dsp_loudness): the result fields, `hop_energy` (numpy [C, hops]
    float64) and `channel_peaks` (numpy [C, 2]: sample, true)."""
    in_ptrs, ref = _rows(x)
    channels, L_ = len(in_ptrs), int(x.shape[1])
    hops = loudness_plan(sr, L_)["hops"]
    z = np.zeros((channels, hops), np.float64)
    peaks = np.zeros((channels, 2), np.float64)
    w, wp = _weights(weights, channels)
    spec = _resample_spec(zeros, beta, rolloff)
    res = L.dsp_loudness_result()
    ex = _exec(ref, 0, stream)
    check(L.lib().dsp_loudness(chan_table(in_ptrs), channels, L_, sr, wp, L.DSP_LOUDNESS_TRUE_PEAK if true_peak else 0,
                               C.byref(spec) if spec is not None else None, _double_rows(z),
                               peaks.ctypes.data_as(C.POINTER(C.c_double)), C.byref(res), C.byref(ex)), "dsp_loudness")
    out = _loudness_dict(res, _LOUDNESS_FIELDS)
    out["hop_energy"], out["channel_peaks"] = z, peaks
    return out


def _limiter_spec(sr, ceiling_db, lookahead_ms, release_ms, true_peak, linked):
    """The limiter's spec from decibels and milliseconds: the ceiling linear in
    float32, the lookahead rounded to whole samples, the release in samples."""
    flags = (L.DSP_LIMITER_TRUE_PEAK if true_peak else 0) | (0 if linked else L.DSP_LIMITER_UNLINKED)
    return L.dsp_limiter_spec(float(np.float32(10.0 ** (ceiling_db / 20.0))), int(round(lookahead_ms * 1e-3 * sr)),
                              release_ms * 1e-3 * sr, flags)


def limiter_plan(sr: int, L_: int = 0, channels: int = 1, ceiling_db: float = -1.0, lookahead_ms: float = 1.5,
                 release_ms: float = 100.0, true_peak: bool = False, linked: bool = True, zeros=None, beta=None,
                 rolloff=None, spec=None) -> dict:
    """dsp_limiter_plan (host only): groups, oversample, rho, the attack window
    (float32 [A + 1]), the ceiling and lookahead it was asked with, and the
    device scratch bytes.  `spec` (a dsp_limiter_spec) overrides the decibel /
    millisecond arguments."""
    sp = spec if spec is not None else _limiter_spec(sr, ceiling_db, lookahead_ms, release_ms, true_peak, linked)
    tp = _resample_spec(zeros, beta, rolloff)
    g, ovs, rho, sb = C.c_uint32(), C.c_uint32(), C.c_float(), C.c_uint64()
    w = np.zeros(min(max(int(sp.lookahead), 0), 1024) + 1, np.float32)
    check(L.lib().dsp_limiter_plan(sr, L_, channels, C.byref(sp), C.byref(tp) if tp is not None else None, C.byref(g),
                                   C.byref(ovs), C.byref(rho), _fp(w), C.byref(sb)), "dsp_limiter_plan")
    return {"groups": g.value, "oversample": ovs.value, "rho": np.float32(rho.value), "window": w,
            "ceiling": np.float32(sp.ceiling), "lookahead": int(sp.lookahead), "scratch_bytes": sb.value}


def limiter(x, sr: int, ceiling_db: float = -1.0, lookahead_ms: float = 1.5, release_ms: float = 100.0,
            true_peak: bool = False, linked: bool = True, return_gain: bool = False, return_detector: bool = False,
            out=None, stream=None, zeros=None, beta=None, rolloff=None, spec=None, result: bool = True):
    """Look-ahead peak limiter over x [C, L] (torch CUDA tensor, or numpy on the
    host) at rate sr (dsp_limiter).  Returns (y, info): y like x (`out`, which
    may be x itself: in place), info with `min_gain` and `limited` (when
    `result`; the call then synchronises), `gain` and `detector` [groups, L]
    where asked.  `spec` (a dsp_limiter_spec) overrides the decibel /
    millisecond arguments."""
    in_ptrs, ref = _rows(x)
    channels, L_ = len(in_ptrs), int(x.shape[1])
    sp = spec if spec is not None else _limiter_spec(sr, ceiling_db, lookahead_ms, release_ms, true_peak, linked)
    groups = channels if sp.flags & L.DSP_LIMITER_UNLINKED else 1
    if out is None:
        out = _alloc_like(ref, (channels, L_))
    out_ptrs, _ = _rows(out)
    gain = _alloc_like(ref, (groups, L_)) if return_gain else None
    det = _alloc_like(ref, (groups, L_)) if return_detector else None
    tp = _resample_spec(zeros, beta, rolloff)
    res = L.dsp_limiter_result()
    ex = _exec(ref, 0, stream)
    check(L.lib().dsp_limiter(chan_table(in_ptrs), channels, L_, chan_table(out_ptrs), sr, C.byref(sp),
                              C.byref(tp) if tp is not None else None,
                              chan_table(_rows(gain)[0]) if return_gain else None,
                              chan_table(_rows(det)[0]) if return_detector else None,
                              C.byref(res) if result else None, C.byref(ex)), "dsp_limiter")
    info = {}
    if result:
        info["min_gain"], info["limited"] = float(res.min_gain), int(res.limited)
    if return_gain:
        info["gain"] = gain
    if return_detector:
        info["detector"] = det
    return out, info


def rfft_plan(n: int) -> dict:
    """dsp_rfft_plan (host only): the passes and radices of the n / 2 point
    complex transform behind an n-point real FFT, and the scratch bytes per channel."""
    p, r, sb = C.c_uint32(), (C.c_uint32 * 4)(), C.c_uint64()
    check(L.lib().dsp_rfft_plan(n, C.byref(p), r, C.byref(sb)), "dsp_rfft_plan")
    return {"passes": p.value, "radix": [int(v) for v in r[:p.value]], "scratch_bytes_per_channel": sb.value}


def rfft(x, n: int, L_: int | None = None, out=None, stream=None):
    """numpy's rfft of the rows of x [C, >= L_] zero-padded to n, a power of two
    in [2^10, 2^24] (dsp_rfft; torch CUDA tensor, or numpy on the host).
    Returns float32 [C, n + 2]: n / 2 + 1 bins of interleaved (re, im)."""
    in_ptrs, ref = _rows(x)
    L_ = int(x.shape[1]) if L_ is None else L_
    if out is None:
        out = _alloc_like(ref, (len(in_ptrs), n + 2))
    out_ptrs, _ = _rows(out)
    ex = _exec(ref, 0, stream)
    check(L.lib().dsp_rfft(chan_table(in_ptrs), len(in_ptrs), L_, n, chan_table(out_ptrs), C.byref(ex)), "dsp_rfft")
    return out


def irfft(spec, n: int, Lout: int | None = None, out=None, stream=None):
    """numpy's irfft of spec [C, n + 2] (n / 2 + 1 bins of interleaved (re, im)),
    the first Lout (default n) samples (dsp_irfft).  Returns float32 [C, Lout]."""
    in_ptrs, ref = _rows(spec)
    Lout = n if Lout is None else Lout
    if out is None:
        out = _alloc_like(ref, (len(in_ptrs), max(Lout, 1)))
    out_ptrs, _ = _rows(out)
    ex = _exec(ref, 0, stream)
    check(L.lib().dsp_irfft(chan_table(in_ptrs), len(in_ptrs), n, chan_table(out_ptrs), Lout, C.byref(ex)), "dsp_irfft")
    return out[:, :Lout]


def deconv_plan(Ly: int, Ls: int, channels: int = 1) -> dict:
    """dsp_deconv_plan (host only): the transform length n and the device scratch bytes."""
    n, sb = C.c_uint32(), C.c_uint64()
    check(L.lib().dsp_deconv_plan(Ly, Ls, channels, C.byref(n), C.byref(sb)), "dsp_deconv_plan")
    return {"n": n.value, "scratch_bytes": sb.value}


def deconvolve(rec, ref, ir_len: int | None = None, eps: float | None = None, pre: int = 0, out=None, stream=None):
    """The impulse responses [C, ir_len] between the excitation ref [Ls] and the
    recordings rec [C, Ly] by regularised spectral division (dsp_deconvolve;
    torch CUDA tensors, or numpy on the host).  The first `pre` samples are
    negative time; ir_len defaults to the plan's n; eps None is the library's 1e-6."""
    in_ptrs, r = _rows(rec)
    Ly, Ls = int(rec.shape[1]), int(ref.shape[0])
    if ir_len is None:
        ir_len = deconv_plan(Ly, Ls, len(in_ptrs))["n"]
    if out is None:
        out = _alloc_like(r, (len(in_ptrs), max(ir_len, 1)))
    out_ptrs, _ = _rows(out)
    ref_ptrs, _ = _rows(ref[None, :] if _is_torch(ref) else np.asarray(ref)[None, :])
    sp = L.dsp_deconv_spec(1e-6 if eps is None else eps, pre)
    ex = _exec(r, 0, stream)
    check(L.lib().dsp_deconvolve(chan_table(in_ptrs), len(in_ptrs), Ly, C.cast(C.c_void_p(ref_ptrs[0]), L.FP), Ls,
                                 chan_table(out_ptrs), ir_len, C.byref(sp) if (eps is not None or pre) else None,
                                 C.byref(ex)), "dsp_deconvolve")
    return out[:, :ir_len]


def _sweep_spec(f1, f2, seconds, amplitude, fade):
    return L.dsp_sweep_spec(f1, f2, seconds, amplitude, fade)


def sweep_plan(sr: int, f1: float, f2: float, seconds: float, amplitude: float = 1.0, fade: int = 0) -> dict:
    """dsp_sweep_plan (host only): the sweep's length L = round(seconds sr) and rate ln(f2 / f1) / seconds."""
    sp = _sweep_spec(f1, f2, seconds, amplitude, fade)
    n, rate = C.c_uint64(), C.c_double()
    check(L.lib().dsp_sweep_plan(sr, C.byref(sp), C.byref(n), C.byref(rate)), "dsp_sweep_plan")
    return {"L": n.value, "rate": rate.value}


def sweep(sr: int, f1: float, f2: float, seconds: float, amplitude: float = 1.0, fade: int = 0):
    """The exponential sine sweep of dsp_sweep (host only): float32 [L]."""
    sp = _sweep_spec(f1, f2, seconds, amplitude, fade)
    x = np.empty(sweep_plan(sr, f1, f2, seconds, amplitude, fade)["L"], np.float32)
    check(L.lib().dsp_sweep(sr, C.byref(sp), _fp(x), x.size), "dsp_sweep")
    return x


def sweep_harmonic_offset(sr: int, f1: float, f2: float, seconds: float, order: int) -> float:
    """Samples by which harmonic order `order`'s response precedes the linear one after deconvolution."""
    sp = _sweep_spec(f1, f2, seconds, 1.0, 0)
    v = C.c_double()
    check(L.lib().dsp_sweep_harmonic_offset(sr, C.byref(sp), order, C.byref(v)), "dsp_sweep_harmonic_offset")
    return v.value


_WELCH_WINDOWS = {"hann": L.DSP_WIN_HANN, "hamming": L.DSP_WIN_HAMMING}


def _welch_spec(hop, window, N=8192):
    w = _WELCH_WINDOWS.get(window, window) if isinstance(window, str) else window
    if isinstance(w, str):
        raise ValueError(f"window {window!r}: 'hann' or 'hamming' (the symmetric tables of stft_magnitude)")
    return L.dsp_welch_spec(N, hop, w)


def welch_plan(L_: int, channels: int = 1, has_ref: bool = False, hop: int = 4096, window="hann", N: int = 8192) -> dict:
    """dsp_welch_plan (host only): frames, bins, the run length of the summation
    order, the device scratch bytes, and the window's sum and sum of squares."""
    sp = _welch_spec(hop, window, N)
    f, b, r, sb, ws, wq = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_double(), C.c_double()
    check(L.lib().dsp_welch_plan(L_, channels, int(has_ref), C.byref(sp), C.byref(f), C.byref(b), C.byref(r),
                                 C.byref(sb), C.byref(ws), C.byref(wq)), "dsp_welch_plan")
    return {"frames": f.value, "bins": b.value, "run": r.value, "scratch_bytes": sb.value, "win_sum": ws.value,
            "win_sumsq": wq.value}


def _f64_like(ref, shape):
    if ref is not None and _is_torch(ref):
        import torch
        return torch.empty(shape, dtype=torch.float64, device=ref.device)
    return np.empty(shape, dtype=np.float64)


def _dptr(a, c=None):
    a = a if c is None else a[c]
    return C.cast(C.c_void_p(a.data_ptr() if _is_torch(a) else a.ctypes.data), L.DP)


def _dtable(a):
    t = (L.DP * max(1, a.shape[0]))()
    for c in range(a.shape[0]):
        t[c] = _dptr(a, c)
    return t


def welch_sums(x, ref=None, hop: int = 4096, window="hann", stream=None):
    """dsp_welch: the raw Welch sums of the rows of x [C, L] (torch CUDA tensor,
    or numpy on the host) over 8192-point frames of hop `hop`, and with the row
    ref [L] the reference's and the cross sums.  Returns float64 (sxx [C, 4097],
    srr [4097] or None, sxy [C, 2 * 4097] interleaved (re, im) or None), where x lives."""
    in_ptrs, r = _rows(x)
    C_, L_, K = len(in_ptrs), int(x.shape[1]), 4097
    sp = _welch_spec(hop, window)
    sxx = _f64_like(r, (C_, K))
    srr = sxy = None
    ref_p = None
    if ref is not None:
        ref_ptrs, _ = _rows(ref[None, :] if _is_torch(ref) else np.asarray(ref)[None, :])
        assert int(ref.shape[0]) == L_, "ref and x must have the same length"
        ref_p = C.cast(C.c_void_p(ref_ptrs[0]), L.FP)
        srr, sxy = _f64_like(r, (K,)), _f64_like(r, (C_, 2 * K))
    ex = _exec(r, 0, stream)
    check(L.lib().dsp_welch(chan_table(in_ptrs), C_, L_, ref_p, _dtable(sxx), _dptr(srr) if ref is not None else None,
                            _dtable(sxy) if ref is not None else None, C.byref(sp), C.byref(ex)), "dsp_welch")
    return sxx, srr, sxy


def welch_derive(sxx, srr, sxy, frames: int, sr: float, win_sum: float, win_sumsq: float, scaling: str = "density",
                 psd: bool = True, cross: bool = True) -> dict:
    """dsp_welch_derive (host only, float64) on numpy sums: {"psd" [C, K],
    "H1" [C, K] complex128, "coherence" [C, K]}, the cross entries only with srr and sxy."""
    if scaling not in ("density", "spectrum"):
        raise ValueError("scaling: 'density' or 'spectrum'")
    sxx = np.ascontiguousarray(sxx, np.float64)
    C_, K = sxx.shape
    cross = cross and srr is not None
    out = {}
    p = np.empty((C_, K)) if psd else None
    h = np.empty((C_, 2 * K)) if cross else None
    g = np.empty((C_, K)) if cross else None
    if cross:
        srr, sxy = np.ascontiguousarray(srr, np.float64), np.ascontiguousarray(sxy, np.float64)
    check(L.lib().dsp_welch_derive(_dtable(sxx), _dptr(srr) if cross else None, _dtable(sxy) if cross else None, C_, K,
                                   frames, sr, win_sum, win_sumsq, L.DSP_WELCH_SPECTRUM if scaling == "spectrum" else 0,
                                   _dtable(p) if psd else None, _dtable(h) if cross else None,
                                   _dtable(g) if cross else None), "dsp_welch_derive")
    if psd:
        out["psd"] = p
    if cross:
        out["H1"] = h.view(np.complex128)
        out["coherence"] = g
    return out


def _welch_host(x, ref, hop, window):
    """The sums of a call on the host as numpy, with the plan."""
    sxx, srr, sxy = welch_sums(x, ref, hop, window)
    if _is_torch(sxx):
        sxx, srr, sxy = (None if a is None else a.cpu().numpy() for a in (sxx, srr, sxy))
    return sxx, srr, sxy, welch_plan(int(x.shape[1]), int(x.shape[0]), ref is not None, hop, window)


def _welch_freqs(sr, K=4097):
    return np.arange(K) * (float(sr) / (2 * (K - 1)))


def welch(x, sr: float, hop: int = 4096, window="hann", scaling: str = "density"):
    """The one-sided average spectrum of the rows of x [C, L]: (freqs [4097],
    psd [C, 4097]) float64 -- scipy.signal.welch(x, sr, w, 8192, 8192 - hop,
    detrend=False, scaling=scaling) with w the library's symmetric window."""
    sxx, _, _, p = _welch_host(x, None, hop, window)
    d = welch_derive(sxx, None, None, p["frames"], sr, p["win_sum"], p["win_sumsq"], scaling)
    return _welch_freqs(sr), d["psd"]


def csd(ref, x, sr: float, hop: int = 4096, window="hann", scaling: str = "density"):
    """The one-sided cross-spectrum between the row ref [L] and the rows of x
    [C, L]: (freqs, pxy [C, 4097] complex128), scipy.signal.csd(ref, x, ...)'s sign and scale."""
    sxx, srr, sxy, p = _welch_host(x, ref, hop, window)
    if scaling not in ("density", "spectrum"):
        raise ValueError("scaling: 'density' or 'spectrum'")
    # dsp_welch_derive has no pxy output: welch_host.cpp welch_derive's psd rule (the scale and
    # the one-sided factors), applied to sxy -- keep the two in step
    den = p["frames"] * (p["win_sum"] ** 2 if scaling == "spectrum" else float(sr) * p["win_sumsq"])
    g = np.full(sxx.shape[1], 2.0)
    g[0] = g[-1] = 1.0
    return _welch_freqs(sr), sxy.view(np.complex128) * (g / den)


def transfer(ref, x, sr: float, hop: int = 4096, window="hann"):
    """The H1 transfer function from the row ref [L] to the rows of x [C, L] and
    its coherence: (freqs, H1 [C, 4097] complex128, coherence [C, 4097])."""
    sxx, srr, sxy, p = _welch_host(x, ref, hop, window)
    d = welch_derive(sxx, srr, sxy, p["frames"], sr, p["win_sum"], p["win_sumsq"], psd=False)
    return _welch_freqs(sr), d["H1"], d["coherence"]


def _stft_window(window):
    w = _WELCH_WINDOWS.get(window, window) if isinstance(window, str) else window
    if isinstance(w, str):
        raise ValueError(f"window {window!r}: 'hann' or 'hamming' (the symmetric tables of stft_magnitude)")
    return w


def stft_plan(L_: int, channels: int = 1, hop: int = 4096, window="hann", N: int = 8192) -> dict:
    """dsp_stft_plan (host only): frames, bins and the least row stride min_ld (floats)."""
    sp = L.dsp_stft_spec(N, hop, _stft_window(window))
    f, b, m = C.c_uint64(), C.c_uint32(), C.c_uint64()
    check(L.lib().dsp_stft_plan(L_, channels, C.byref(sp), C.byref(f), C.byref(b), C.byref(m)), "dsp_stft_plan")
    return {"frames": f.value, "bins": b.value, "min_ld": m.value}


def istft_plan(frames: int, channels: int = 1, hop: int = 4096, window="hann", floor: float = 1e-10,
               N: int = 8192) -> dict:
    """dsp_istft_plan (host only): the full output length N + (F - 1) hop, the
    frames that touch a sample, the frames per chunk and the device scratch bytes."""
    sp = L.dsp_istft_spec(N, hop, _stft_window(window), floor)
    lo, ov, ch, sb = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    check(L.lib().dsp_istft_plan(frames, channels, C.byref(sp), C.byref(lo), C.byref(ov), C.byref(ch), C.byref(sb)),
          "dsp_istft_plan")
    return {"Lout": lo.value, "overlap": ov.value, "chunk": ch.value, "scratch_bytes": sb.value}


def _complex_rows(z):
    """A complex64 [C, F, K] buffer (torch CUDA or numpy, unit stride along K) as
    (row pointers, the buffer, F, ld in floats)."""
    if _is_torch(z):
        import torch
        assert z.dtype == torch.complex64 and z.dim() == 3 and z.stride(2) == 1
        assert z.shape[1] == 1 or z.stride(1) >= z.shape[2]
        return [z[c].data_ptr() for c in range(z.shape[0])], z, int(z.shape[1]), 2 * int(z.stride(1))
    z = np.asarray(z)
    assert z.dtype == np.complex64 and z.ndim == 3 and z.strides[2] == 8 and z.strides[1] % 8 == 0
    return [z[c].ctypes.data for c in range(z.shape[0])], z, int(z.shape[1]), z.strides[1] // 4


def stft(x, hop: int = 4096, window="hann", out=None, stream=None):
    """The complex STFT of the rows of x [C, L] (dsp_stft; torch CUDA tensor, or
    numpy on the host) over 8192-point frames of hop `hop` under the library's
    symmetric window, unnormalised: complex64 [C, F, 4097], where x lives.
    torch.stft(x, 8192, hop, window=w, center=False, return_complex=True), with
    w that window table, is this result transposed to [C, 4097, F]."""
    in_ptrs, ref = _rows(x)
    C_, L_, K = len(in_ptrs), int(x.shape[1]), 4097
    sp = L.dsp_stft_spec(8192, hop, _stft_window(window))
    F = stft_plan(L_, C_, hop, window)["frames"]
    if out is None:
        if _is_torch(ref):
            import torch
            out = torch.empty((C_, F, K), dtype=torch.complex64, device=ref.device)
        else:
            out = np.empty((C_, F, K), np.complex64)
    out_ptrs, _, Fo, ld = _complex_rows(out)
    assert out.shape[0] == C_ and Fo == F and out.shape[2] == K
    ex = _exec(ref, 0, stream)
    check(L.lib().dsp_stft(chan_table(in_ptrs), C_, L_, chan_table(out_ptrs), ld if F > 1 else max(ld, 2 * K),
                           C.byref(sp), C.byref(ex)), "dsp_stft")
    return out


def istft(Z, hop: int = 4096, window="hann", length: int | None = None, floor: float = 1e-10, out=None, stream=None):
    """The least-squares overlap-add inverse of a complex spectrogram Z
    [C, F, 4097] complex64 (dsp_istft; torch CUDA tensor, or numpy on the host)
    with the analysis window for synthesis: float32 [C, length], length
    defaulting to 8192 + (F - 1) hop; 512 <= hop <= 8192.  A sample whose sum of
    squared window values is below `floor` is 0.  istft(stft(x)) is x wherever
    that sum is not; torch.istft(Z^T, 8192, hop, window=w, center=False) computes
    the same where its own envelope check lets it (a Hann window's zero ends fail it)."""
    ptrs, ref, F, ld = _complex_rows(Z)
    C_ = len(ptrs)
    assert Z.shape[2] == 4097
    sp = L.dsp_istft_spec(8192, hop, _stft_window(window), floor)
    full = istft_plan(F, C_, hop, window, floor)["Lout"]
    length = full if length is None else length
    if out is None:
        out = _alloc_like(ref if _is_torch(ref) else None, (C_, max(length, 1)))
    out_ptrs, _ = _rows(out)
    ex = _exec(ref if _is_torch(ref) else None, 0, stream)
    check(L.lib().dsp_istft(chan_table(ptrs), C_, F, ld if F > 1 else max(ld, 2 * 4097), chan_table(out_ptrs), length,
                            C.byref(sp), C.byref(ex)), "dsp_istft")
    return out[:, :length]


def pvoc_plan(frames: int, rate: float, channels: int = 1) -> dict:
    """dsp_pvoc_plan (host only): the output frames of `frames` input frames at
    `rate`, the output frames per chunk and the device scratch bytes."""
    sp = L.dsp_pvoc_spec(rate)
    fo, ch, sb = C.c_uint64(), C.c_uint32(), C.c_uint64()
    check(L.lib().dsp_pvoc_plan(frames, channels, C.byref(sp), C.byref(fo), C.byref(ch), C.byref(sb)), "dsp_pvoc_plan")
    return {"frames": fo.value, "chunk": ch.value, "scratch_bytes": sb.value}


def phase_vocoder(Z, rate: float, out=None, stream=None):
    """The phase vocoder on a complex spectrogram Z [C, F, 4097] complex64
    (dsp_pvoc; torch CUDA tensor, or numpy on the host): complex64
    [C, F', 4097] where Z lives, F' = pvoc_plan(F, rate)["frames"]; rate > 1
    shortens.  librosa.phase_vocoder(Z^T, rate=rate)'s recurrence, the phase
    carried as a 32-bit fixed-point fraction of a turn."""
    ptrs, ref, F, ld = _complex_rows(Z)
    C_, K = len(ptrs), 4097
    assert Z.shape[2] == K
    sp = L.dsp_pvoc_spec(rate)
    Fo = pvoc_plan(F, rate, C_)["frames"]
    if out is None:
        if _is_torch(ref):
            import torch
            out = torch.empty((C_, Fo, K), dtype=torch.complex64, device=ref.device)
        else:
            out = np.empty((C_, Fo, K), np.complex64)
    out_ptrs, _, Fout, ld_out = _complex_rows(out)
    assert out.shape[0] == C_ and Fout == Fo and out.shape[2] == K
    ex = _exec(ref if _is_torch(ref) else None, 0, stream)
    check(L.lib().dsp_pvoc(chan_table(ptrs), C_, F, ld if F > 1 else max(ld, 2 * K), chan_table(out_ptrs),
                           ld_out if Fo > 1 else max(ld_out, 2 * K), C.byref(sp), C.byref(ex)), "dsp_pvoc")
    return out


def _stretch_spec(rate, hop, window, floor):
    return L.dsp_stretch_spec(rate, 8192, hop, _stft_window(window), floor)


def time_stretch_plan(L_: int, rate: float, channels: int = 1, hop: int = 2048, window="hann",
                      floor: float = 1e-10) -> dict:
    """dsp_time_stretch_plan (host only): frames in and out, the full and the
    default output length, and the bytes of the two device spectrograms."""
    sp = _stretch_spec(rate, hop, window, floor)
    fi, fo, lf, ld, db = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(L.lib().dsp_time_stretch_plan(L_, channels, C.byref(sp), C.byref(fi), C.byref(fo), C.byref(lf), C.byref(ld),
                                        C.byref(db)), "dsp_time_stretch_plan")
    return {"frames_in": fi.value, "frames_out": fo.value, "Lout_full": lf.value, "Lout": ld.value,
            "device_bytes": db.value}


def time_stretch(x, rate: float, hop: int = 2048, window="hann", length: int | None = None, floor: float = 1e-10,
                 out=None, stream=None):
    """x [C, L] (torch CUDA tensor, or numpy on the host) made 1 / rate times as
    long at the same pitch (dsp_time_stretch: stft, phase_vocoder, istft at hop
    `hop`): float32 [C, length], length defaulting to round(L / rate) (at most
    the plan's Lout_full)."""
    in_ptrs, ref = _rows(x)
    C_, L_ = len(in_ptrs), int(x.shape[1])
    p = time_stretch_plan(L_, rate, C_, hop, window, floor)
    length = p["Lout"] if length is None else length
    if out is None:
        out = _alloc_like(ref, (C_, max(length, 1)))
    out_ptrs, _ = _rows(out)
    sp = _stretch_spec(rate, hop, window, floor)
    ex = _exec(ref, 0, stream)
    check(L.lib().dsp_time_stretch(chan_table(in_ptrs), C_, L_, chan_table(out_ptrs), length, C.byref(sp),
                                   C.byref(ex)), "dsp_time_stretch")
    return out[:, :length]


def pitch_ratio(semitones: float) -> tuple[int, int]:
    """dsp_pitch_ratio (host only): (p, q), p / q the best approximation of
    2^(semitones / 12) with p, q <= 4096."""
    p, q = C.c_uint32(), C.c_uint32()
    check(L.lib().dsp_pitch_ratio(semitones, C.byref(p), C.byref(q)), "dsp_pitch_ratio")
    return p.value, q.value


def pitch_shift_plan(L_: int, semitones: float, channels: int = 1, hop: int = 2048, window="hann") -> dict:
    """dsp_pitch_shift_plan (host only): (p, q) = pitch_ratio(semitones), rate = q / p,
    `stretched` = floor(L_ p / q + 1 / 2), `padded` = the least max(L_, 8192) + j hop whose
    time_stretch_plan reaches `stretched` samples -- a stretch to a longer row ends
    (8192 - hop) (1 / rate - 1) samples early without it -- and Lout = resample_plan's
    length of `stretched` samples from p to q, within a sample of L_."""
    p, q, sp = C.c_uint32(), C.c_uint32(), L.dsp_stretch_spec()
    pad, st, lo = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(L.lib().dsp_pitch_shift_plan(L_, channels, semitones, hop, _stft_window(window), C.byref(p), C.byref(q),
                                       C.byref(sp), C.byref(pad), C.byref(st), C.byref(lo)), "dsp_pitch_shift_plan")
    return {"p": p.value, "q": q.value, "rate": sp.rate, "padded": pad.value, "stretched": st.value, "Lout": lo.value}


def pitch_shift(x, semitones: float, hop: int = 2048, window="hann"):
    """x [C, L] shifted by `semitones` at (within a sample) the same length, by the two public
    calls: with pl = pitch_shift_plan(L, semitones), x zero-padded to pl["padded"] samples,
    time_stretch(., pl["rate"], length=pl["stretched"]) and resample(., p, q)."""
    L_ = int(x.shape[1])
    pl = pitch_shift_plan(L_, semitones, int(x.shape[0]), hop, window)
    if pl["padded"] > L_:
        if _is_torch(x):
            import torch
            x = torch.nn.functional.pad(x, (0, pl["padded"] - L_))
        else:
            x = np.pad(np.asarray(x), ((0, 0), (0, pl["padded"] - L_)))
    return resample(time_stretch(x, pl["rate"], hop, window, length=pl["stretched"]), pl["p"], pl["q"])


_DECAY_BANDS = {"octave": (1, -5, 4), "third": (3, -16, 13)}
_DECAY_FIELDS = ("edt", "t20", "t30", "c50", "c80", "d50", "ts", "inr")


def decay_plan(L_: int, sr: int, fraction: int = 1, k_lo: int = -5, k_hi: int = 4, channels: int = 1) -> dict:
    """dsp_decay_plan (host only): the transform size n, the padding P, hop, the
    band count, the length `hops` of an energy row, the device scratch bytes and
    the bands' mid frequencies fm."""
    sp = L.dsp_decay_spec(fraction, k_lo, k_hi)
    n, P, hop, bands, hops, sb = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
    fm = (C.c_double * 32)()
    check(L.lib().dsp_decay_plan(L_, channels, sr, C.byref(sp), C.byref(n), C.byref(P), C.byref(hop), C.byref(bands),
                                 C.byref(hops), C.byref(sb), fm), "dsp_decay_plan")
    return {"n": n.value, "P": P.value, "hop": hop.value, "bands": bands.value, "hops": hops.value,
            "scratch_bytes": sb.value, "fm": np.array(fm[:bands.value])}


def decay_energies(x, sr: int, fraction: int = 1, k_lo: int = -5, k_hi: int = 4, moments: bool = True, stream=None):
    """dsp_decay: the hop energies of the band-filtered rows of x [C, L] (torch
    CUDA tensor, or numpy on the host).  Returns (peak [C] float32, onset [C]
    uint64 (int64 on torch), energy [C, bands, hops] float64, moment likewise or
    None), where x lives."""
    in_ptrs, r = _rows(x)
    C_, L_ = len(in_ptrs), int(x.shape[1])
    p = decay_plan(L_, sr, fraction, k_lo, k_hi, C_)
    B, hops = p["bands"], p["hops"]
    sp = L.dsp_decay_spec(fraction, k_lo, k_hi)
    energy = _f64_like(r, (C_ * B, hops))
    moment = _f64_like(r, (C_ * B, hops)) if moments else None
    if _is_torch(r):
        import torch
        peak = torch.empty((C_,), dtype=torch.float32, device=r.device)
        onset = torch.empty((C_,), dtype=torch.int64, device=r.device)
        pp, po = peak.data_ptr(), onset.data_ptr()
    else:
        peak, onset = np.empty(C_, np.float32), np.empty(C_, np.uint64)
        pp, po = peak.ctypes.data, onset.ctypes.data
    ex = _exec(r, 0, stream)
    check(L.lib().dsp_decay(chan_table(in_ptrs), C_, L_, sr, C.byref(sp), C.cast(C.c_void_p(pp), L.FP),
                            C.cast(C.c_void_p(po), C.POINTER(C.c_uint64)), _dtable(energy),
                            _dtable(moment) if moments else None, C.byref(ex)), "dsp_decay")
    shape = (C_, B, hops)
    return peak, onset, energy.reshape(shape), (moment.reshape(shape) if moments else None)


def decay_derive(energy, moment, L_: int, onset: int, hop: int, sr: int) -> dict:
    """dsp_decay_derive (host only, float64) on one energy row (and its moment
    row, or None): edt, t20, t30, c50, c80, d50, ts, inr, flags, truncation."""
    e = np.ascontiguousarray(energy, np.float64)
    m = None if moment is None else np.ascontiguousarray(moment, np.float64)
    assert e.ndim == 1 and e.shape[0] == (L_ + hop - 1) // hop + 1 and (m is None or m.shape == e.shape)
    res = L.dsp_decay_result()
    check(L.lib().dsp_decay_derive(_dptr(e), None if m is None else _dptr(m), L_, int(onset), hop, sr, C.byref(res)),
          "dsp_decay_derive")
    out = {k: getattr(res, k) for k in _DECAY_FIELDS}
    out["flags"], out["truncation"] = res.flags, res.truncation
    return out


def decay(ir, sr: int, bands="octave") -> dict:
    """The ISO 3382 figures of the impulse responses ir [C, L] per band: a dict of
    float64 arrays [C, bands] (edt, t20, t30 in seconds, c50, c80 in dB, d50, ts
    in seconds, inr in dB; NaN where not derivable) and flags [C, bands], plus fm
    [bands] in Hz, onset [C], peak [C] and hop.  bands: 'octave' (31.6 Hz..16 kHz),
    'third' (25 Hz..20 kHz), each without the bands whose upper edge lies above
    sr / 2, or (fraction, k_lo, k_hi) as given."""
    if isinstance(bands, str):
        if bands not in _DECAY_BANDS:
            raise ValueError(f"bands {bands!r}: 'octave', 'third' or (fraction, k_lo, k_hi)")
        fraction, k_lo, k_hi = _DECAY_BANDS[bands]
        while k_hi > k_lo and 1000.0 * 10.0 ** (0.3 * (k_hi + 0.5) / fraction) > 0.5 * sr:
            k_hi -= 1
    else:
        fraction, k_lo, k_hi = bands
    L_ = int(ir.shape[1])
    p = decay_plan(L_, sr, fraction, k_lo, k_hi, int(ir.shape[0]))
    peak, onset, energy, moment = decay_energies(ir, sr, fraction, k_lo, k_hi)
    if _is_torch(energy):
        peak, onset, energy, moment = (a.cpu().numpy() for a in (peak, onset, energy, moment))
    C_, B = energy.shape[:2]
    out = {k: np.empty((C_, B)) for k in _DECAY_FIELDS}
    out["flags"] = np.zeros((C_, B), np.uint32)
    for c in range(C_):
        for b in range(B):
            d = decay_derive(energy[c, b], moment[c, b], L_, int(onset[c]), p["hop"], sr)
            for k in _DECAY_FIELDS:
                out[k][c, b] = d[k]
            out["flags"][c, b] = d["flags"]
    out["fm"], out["onset"], out["peak"], out["hop"] = p["fm"], onset.astype(np.uint64), peak, p["hop"]
    return out


def stft_frames(L_: int, N: int, H: int) -> int:
    return int(L.lib().dsp_stft_frame_count(L_, N, H))


def num_blocks(L_: int, B: int) -> int:
    return (L_ + B - 1) // B


# --------------------------------------------------------------------------
# entry points
# --------------------------------------------------------------------------

_tls = threading.local()


def last_result() -> int:
    """dsp_exec.result of this thread's last render_offline / render_stft /
    render_loop / render_stft_host (DSP_RESULT_CLASS / _VERIFIED / _RERENDERED /
    _FRAME_REUSE bits; the chunked driver ORs its chunks' bits)."""
    return getattr(_tls, "result", 0)


def _track(ex):
    r = C.c_uint32(0)
    ex.result = C.pointer(r)
    return r


def render_offline(file, C_out: int, B: int, sr: float, plugin: Plugin | None,
                   out=None, sample_offset: int = 0, L_file: int | None = None, stream=None):
    """Offline one-shot render.  file: [Cin, L] (Cin may be 0 / None).
    Returns out: [C_out, ceil(L/B)*B]."""
    in_ptrs, ref = _rows(file)
    L_ = L_file if L_file is not None else (file.shape[1] if file is not None else 0)
    nb = num_blocks(L_, B)
    if out is None:
        out = _alloc_like(ref, (C_out, max(nb * B, 1)))
    out_ptrs, oref = _rows(out)
    ex = _exec(oref, sample_offset, stream)
    ps = plugin.as_struct() if plugin is not None else None
    ex.flags |= plugin.exec_flags if plugin is not None else 0
    res = _track(ex)
    st = L.lib().dsp_render_offline(chan_table(in_ptrs) if in_ptrs else None, len(in_ptrs), L_,
                                    chan_table(out_ptrs), C_out, B, sr,
                                    C.byref(ps) if ps is not None else None, C.byref(ex))
    check(st, "dsp_render_offline")
    _tls.result = res.value
    return out[:, : nb * B]


def render_loop(file, C_out: int, B: int, nblocks: int, sr: float, plugin: Plugin | None,
                cursor: int = 0, out=None, sample_offset: int = 0, stream=None):
    """Loop-mode render (audio.cpp:100-132): the file wraps from `cursor`.
    Device tensors only.  Returns (out [C_out, nblocks*B], next cursor)."""
    in_ptrs, ref = _rows(file)
    L_ = file.shape[1] if file is not None else 0
    if out is None:
        out = _alloc_like(ref, (C_out, max(nblocks * B, 1)))
    out_ptrs, oref = _rows(out)
    ex = _exec(oref, sample_offset, stream)
    ps = plugin.as_struct() if plugin is not None else None
    ex.flags |= plugin.exec_flags if plugin is not None else 0
    res = _track(ex)
    cur = C.c_uint64()
    st = L.lib().dsp_render_loop(chan_table(in_ptrs) if in_ptrs else None, len(in_ptrs), L_, cursor,
                                 chan_table(out_ptrs), C_out, B, nblocks, sr,
                                 C.byref(ps) if ps is not None else None, C.byref(cur), C.byref(ex))
    check(st, "dsp_render_loop")
    _tls.result = res.value
    return out[:, : nblocks * B], cur.value


def stft_magnitude(x, N: int = 8192, H: int = 4096, window: int = L.DSP_WIN_HANN,
                   K: int | None = None, ld: int | None = None, out=None, L_sig: int | None = None,
                   stream=None):
    """STFT magnitudes of x: [C, L] -> [C, F, K]."""
    in_ptrs, ref = _rows(x)
    K = K if K is not None else N // 2 + 1
    ld = ld if ld is not None else K
    L_ = L_sig if L_sig is not None else x.shape[1]
    F = stft_frames(L_, N, H)
    if out is None:
        out = _alloc_like(ref, (len(in_ptrs), max(F, 1), ld))
    mag_ptrs = [out[c].data_ptr() if _is_torch(out) else out[c].ctypes.data for c in range(len(in_ptrs))]
    ex = _exec(ref, 0, stream)
    st = L.lib().dsp_stft_magnitude(chan_table(in_ptrs), len(in_ptrs), L_, N, H, window, K,
                                    chan_table(mag_ptrs), ld, C.byref(ex))
    check(st, "dsp_stft_magnitude")
    return out[:, :F, :K]


def render_stft(file, C_out: int, B: int, sr: float, plugin: Plugin | None,
                N: int = 8192, H: int = 4096, window: int = L.DSP_WIN_HANN, K: int | None = None,
                ld: int | None = None, out=None, mag=None, sample_offset: int = 0,
                L_file: int | None = None, ref=None, stream=None):
    """Render + STFT of the render.  Returns (out [C, nblocks*B], mag [C, F, K])."""
    in_ptrs, r = _rows(file)
    ref = r if r is not None else ref
    L_ = L_file if L_file is not None else (file.shape[1] if file is not None else 0)
    nb = num_blocks(L_, B)
    K = K if K is not None else N // 2 + 1
    ld = ld if ld is not None else K
    F = stft_frames(nb * B, N, H)
    if out is None:
        out = _alloc_like(ref, (C_out, max(nb * B, 1)))
    if mag is None:
        mag = _alloc_like(ref, (C_out, max(F, 1), ld))
    out_ptrs, oref = _rows(out)
    mag_ptrs = [mag[c].data_ptr() if _is_torch(mag) else mag[c].ctypes.data for c in range(C_out)]
    ex = _exec(oref, sample_offset, stream)
    ps = plugin.as_struct() if plugin is not None else None
    ex.flags |= plugin.exec_flags if plugin is not None else 0
    res = _track(ex)
    st = L.lib().dsp_render_stft(chan_table(in_ptrs) if in_ptrs else None, len(in_ptrs), L_,
                                 chan_table(out_ptrs), C_out, B, sr,
                                 C.byref(ps) if ps is not None else None, N, H, window, K,
                                 chan_table(mag_ptrs), ld, C.byref(ex))
    check(st, "dsp_render_stft")
    _tls.result = res.value
    return out[:, : nb * B], mag[:, :F, :K]


def render_stft_host(x, C_out: int, B: int, sr: float, plugin: Plugin | None, stft: bool = True,
                     N: int = 8192, H: int = 4096, window: int = L.DSP_WIN_HANN, K: int | None = None,
                     chunk: int = 1 << 22, out=None, mag=None, sample_offset: int = 0, device: int = -1,
                     stream=None):
    """Host rows in, host rows out, streamed through HBM in chunks
    (dsp_render_stft_host).  x: numpy / pinned torch CPU [Cin, L] float32.
    Returns (out [C_out, ceil(L/B)B], mag [C_out, F, K] | None)."""
    K = K if K is not None else N // 2 + 1
    L_ = int(x.shape[1]) if x is not None else 0
    Lp = num_blocks(L_, B) * B
    F = stft_frames(Lp, N, H) if stft else 0
    out = np.empty((C_out, max(Lp, 1)), np.float32) if out is None else out
    if stft and mag is None:
        mag = np.empty((C_out, max(F, 1), K), np.float32)
    ptr = lambda a, c: a[c].data_ptr() if _is_torch(a) else a[c].ctypes.data  # noqa: E731
    in_ptrs = [ptr(x, c) for c in range(x.shape[0])] if x is not None else []
    ex = dsp_exec(device, 0, C.c_void_p(stream) if stream else None, sample_offset)
    ps = plugin.as_struct() if plugin is not None else None
    ex.flags |= plugin.exec_flags if plugin is not None else 0
    res = _track(ex)
    st = L.lib().dsp_render_stft_host(chan_table(in_ptrs) if in_ptrs else None, len(in_ptrs), L_,
                                      chan_table([ptr(out, c) for c in range(C_out)]), C_out, B, sr,
                                      C.byref(ps) if ps is not None else None, N, H, window, K,
                                      chan_table([ptr(mag, c) for c in range(C_out)]) if stft else None, K, chunk,
                                      C.byref(ex))
    check(st, "dsp_render_stft_host")
    _tls.result = res.value
    return out[:, :Lp], (mag[:, :F] if stft else None)


def ir_analysis(plugin: Plugin | None, C_out: int = 2, sr: float = 48000.0,
                ir_len: int = IR_BUFFER_LENGTH, device=None):
    """compute_IR + fft_perform_and_get_magnitude.  Returns (ir [C, ir_len],
    mag [4*ir_len]) as torch tensors on `device`, or numpy when device is None."""
    if device is not None:
        import torch
        ir = torch.empty((C_out, ir_len), dtype=torch.float32, device=device)
        mag = torch.empty((4 * ir_len,), dtype=torch.float32, device=device)
        ir_ptrs = [ir[c].data_ptr() for c in range(C_out)]
        mptr = mag.data_ptr()
        ex = _exec(ir)
    else:
        ir = np.empty((C_out, ir_len), np.float32)
        mag = np.empty((4 * ir_len,), np.float32)
        ir_ptrs = [ir[c].ctypes.data for c in range(C_out)]
        mptr = mag.ctypes.data
        ex = _exec(None)
    ps = plugin.as_struct() if plugin is not None else None
    ex.flags |= plugin.exec_flags if plugin is not None else 0
    st = L.lib().dsp_ir_analysis(C.byref(ps) if ps is not None else None, C_out, sr, ir_len,
                                 chan_table(ir_ptrs), C.cast(C.c_void_p(mptr), L.FP), C.byref(ex))
    check(st, "dsp_ir_analysis")
    return ir, mag


def _fp(a):
    return C.cast(C.c_void_p(a.data_ptr() if _is_torch(a) else a.ctypes.data), L.FP)


def fft_forward(x):
    """fft_forward (dsp.cpp:74-103): real n -> (re, im), 1/sqrt(n) scaling."""
    n = x.shape[0]
    re, im = _alloc_like(x if _is_torch(x) else None, (n,)), _alloc_like(x if _is_torch(x) else None, (n,))
    ex = _exec(x if _is_torch(x) else None)
    check(L.lib().dsp_fft_forward(_fp(x), _fp(re), _fp(im), n, C.byref(ex)), "dsp_fft_forward")
    return re, im


def fft_reverse(re, im):
    """fft_reverse (dsp.cpp:106-132): Re(IDFT)/sqrt(n)."""
    n = re.shape[0]
    out = _alloc_like(re if _is_torch(re) else None, (n,))
    ex = _exec(re if _is_torch(re) else None)
    check(L.lib().dsp_fft_reverse(_fp(re), _fp(im), _fp(out), n, C.byref(ex)), "dsp_fft_reverse")
    return out


# --------------------------------------------------------------------------
# display reductions (long-file overviews)
# --------------------------------------------------------------------------

def minmax_decimate(x, pixels: int):
    """Per-pixel (max, min) of a 1-D signal, the reference's IR view
    (opengl.h:877-890).  Returns (vmax [pixels], vmin [pixels])."""
    ref = x if _is_torch(x) else None
    vmax = _alloc_like(ref, (max(pixels, 1),))
    vmin = _alloc_like(ref, (max(pixels, 1),))
    ex = _exec(ref)
    st = L.lib().dsp_minmax_decimate(_fp(x), x.shape[0], pixels, _fp(vmax), _fp(vmin), C.byref(ex))
    check(st, "dsp_minmax_decimate")
    return vmax[:pixels], vmin[:pixels]


def spectrogram_decimate(mag, pixels: int):
    """[F, K] magnitudes (row stride = mag's) -> [pixels, K] column maxima."""
    ref = mag if _is_torch(mag) else None
    F, K = int(mag.shape[0]), int(mag.shape[1])
    ld = (mag.stride(0) if _is_torch(mag) else mag.strides[0] // 4)
    out = _alloc_like(ref, (max(pixels, 1), K))
    ex = _exec(ref)
    st = L.lib().dsp_spectrogram_decimate(_fp(mag), F, K, ld, pixels, _fp(out), C.byref(ex))
    check(st, "dsp_spectrogram_decimate")
    return out[:pixels]
