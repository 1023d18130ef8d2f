"""Which row layouts the Plugin-free row calls refuse (csrc/capi_signal.cpp,
the overlap predicates of csrc/host_hip.hpp).

Rows are views into one float32 array, passed as host buffers: a refused
layout returns DSP_ERR_INVALID with the call's text before any device is
looked at; an accepted one gets as far as the device (DSP_ERR_NO_DEVICE
without a GPU, DSP_OK with one, where it computes on memory the test owns).
Lengths are the smallest the plans allow: rows of 64 samples, n = 1024.
"""
import ctypes as C

import numpy as np
import pytest

import dspbench as d
from dspbench import _lib

L64, N, BINS2 = 64, 1024, 1024 + 2
SR = 48000
FLOATS = 8192

TEXT = {
    "resample": b"dsp_resample: output rows overlap input rows",
    "limiter": b"dsp_limiter: rows overlap (only out[c] == in[c] is allowed)",
    "rfft": b"dsp_rfft: spectrum rows overlap input rows or each other",
    "irfft": b"dsp_irfft: output rows overlap spectrum rows or each other",
    "deconvolve": b"dsp_deconvolve: ir rows overlap rec, ref or each other",
}
# floats of an input row and of an output row
LENS = {"resample": (L64, 2 * L64), "limiter": (L64, L64), "rfft": (L64, BINS2), "irfft": (BINS2, L64),
        "deconvolve": (L64, L64)}
CALLS = sorted(LENS)
REF_AT = 7000  # dsp_deconvolve's excitation, clear of every layout below


@pytest.fixture()
def buf():
    return np.random.default_rng(7).uniform(-0.5, 0.5, FLOATS).astype(np.float32)


def _rows(buf, offsets):
    for o in offsets:
        assert 0 <= o < FLOATS
    return _lib.chan_table([buf.ctypes.data + 4 * o for o in offsets])


def _ex():
    return _lib.dsp_exec(-1, _lib.DSP_EXEC_HOST_BUFFERS, None, 0, None)


def _call(buf, call, a, b, *, L=None, gain=None, det=None, unlinked=False, ref=REF_AT, null_in=False):
    """One call with input rows at float offsets `a` and output rows at `b`."""
    lib = d.lib()
    la, lb = LENS[call]
    for o in list(a) + list(b):
        assert o + max(la, lb) <= FLOATS
    ex = _ex()
    A = (_lib.FP * 2)() if null_in else _rows(buf, a)
    B = _rows(buf, b)
    if call == "resample":
        Lout = C.c_uint64(0)
        assert lib.dsp_resample_plan(SR, 2 * SR, L64, None, None, None, None, C.byref(Lout), None) == 0
        assert Lout.value == lb
        return lib.dsp_resample(A, 2, L64, B, lb, SR, 2 * SR, None, C.byref(ex))
    if call == "limiter":
        spec = _lib.dsp_limiter_spec(0.25, 0, 0.0, _lib.DSP_LIMITER_UNLINKED if unlinked else 0)
        return lib.dsp_limiter(A, 2, L64, B, SR, C.byref(spec), None, _rows(buf, gain) if gain else None,
                               _rows(buf, det) if det else None, None, C.byref(ex))
    if call == "rfft":
        return lib.dsp_rfft(A, 2, L64 if L is None else L, N, B, C.byref(ex))
    if call == "irfft":
        return lib.dsp_irfft(A, 2, N, B, L64, C.byref(ex))
    assert call == "deconvolve"
    assert ref + L64 <= FLOATS
    return lib.dsp_deconvolve(A, 2, L64, C.cast(C.c_void_p(buf.ctypes.data + 4 * ref), _lib.FP), L64, B, L64, None,
                              C.byref(ex))


def _refused(call, st):
    assert st == _lib.DSP_ERR_INVALID, (st, d.lib().dsp_last_error())
    assert d.lib().dsp_last_error() == TEXT[call]


def _accepted(st):
    assert st != _lib.DSP_ERR_INVALID, d.lib().dsp_last_error()


@pytest.mark.parametrize("call", CALLS)
def test_adjacent_rows_are_accepted(buf, call):
    la, lb = LENS[call]
    _accepted(_call(buf, call, [0, la], [2 * la, 2 * la + lb]))


@pytest.mark.parametrize("call", CALLS)
def test_one_float_of_overlap_is_refused(buf, call):
    la, lb = LENS[call]
    _refused(call, _call(buf, call, [0, la], [2 * la - 1, 2 * la - 1 + lb]))


@pytest.mark.parametrize("call", CALLS)
def test_output_shifted_by_8_floats_is_refused(buf, call):
    la, lb = LENS[call]
    S = la + lb + 16
    _refused(call, _call(buf, call, [0, S], [8, S + 8]))


@pytest.mark.parametrize("call", CALLS)
def test_in_place_is_for_the_limiter_only(buf, call):
    S = max(LENS[call])
    st = _call(buf, call, [0, S], [0, S])
    if call == "limiter":
        _accepted(st)
    else:
        _refused(call, st)


@pytest.mark.parametrize("call", CALLS)
def test_output_row_on_another_channels_input_is_refused(buf, call):
    S = max(LENS[call])
    _refused(call, _call(buf, call, [0, S], [S, 2 * S]))  # out[0] == in[1]


@pytest.mark.parametrize("call", CALLS)
def test_two_equal_output_rows(buf, call):
    la, lb = LENS[call]
    st = _call(buf, call, [0, la], [2 * la, 2 * la])
    if call == "resample":  # (not looked at: each host row is staged on its own)
        _accepted(st)
    else:
        _refused(call, st)


# rows of the limiter at 0 / 64 (in), 128 / 192 (out), free from 256 on
@pytest.mark.parametrize("kw", [
    dict(gain=[32]),                                    # against in
    dict(gain=[128 + 63]),                              # against out
    dict(gain=[256], det=[256 + 63]),                   # against the detector row
    dict(gain=[256], det=[256]),
    dict(det=[64 + 63]),                                # the detector row against in
    dict(gain=[256, 256 + 63], unlinked=True),          # an unlinked spec's gain rows against each other
    dict(det=[256, 256], unlinked=True),
], ids=["gain-in", "gain-out", "gain-det", "gain-is-det", "det-in", "gain-gain", "det-det"])
def test_limiter_gain_and_detector_rows_refused(buf, kw):
    _refused("limiter", _call(buf, "limiter", [0, 64], [128, 192], **kw))


@pytest.mark.parametrize("kw", [
    dict(gain=[256], det=[320]),
    dict(gain=[256, 320], det=[384, 448], unlinked=True),
], ids=["linked", "unlinked"])
def test_limiter_adjacent_gain_and_detector_rows_accepted(buf, kw):
    _accepted(_call(buf, "limiter", [0, 64], [128, 192], **kw))


def test_deconvolve_ref_against_ir_is_refused(buf):
    _refused("deconvolve", _call(buf, "deconvolve", [0, 64], [128, 192], ref=192 + 63))
    _accepted(_call(buf, "deconvolve", [0, 64], [128, 192], ref=256))
    # rec and ref are only read: they may share memory
    _accepted(_call(buf, "deconvolve", [0, 64], [128, 192], ref=0))


def test_rfft_next_row_inside_a_spectrums_last_bin_is_refused(buf):
    # a spectrum is n + 2 floats: rows n floats apart share the Nyquist bin
    _refused("rfft", _call(buf, "rfft", [0, 64], [128, 128 + N]))
    _refused("rfft", _call(buf, "rfft", [0, 64], [128, 128 + N + 1]))
    _accepted(_call(buf, "rfft", [0, 64], [128, 128 + BINS2]))


def test_rfft_of_no_samples_does_not_look_at_in(buf):
    _accepted(_call(buf, "rfft", [], [0, BINS2], L=0, null_in=True))
    # ... but its spectrum rows still may not overlap
    _refused("rfft", _call(buf, "rfft", [], [0, N], L=0, null_in=True))
