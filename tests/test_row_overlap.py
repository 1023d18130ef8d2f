"""Which row layouts the Plugin-free row calls refuse (csrc/capi_rate.cpp,
capi_bigfft.cpp and capi_grid.cpp; the overlap predicates and the one layout
rule, output_rows_overlap, of csrc/host_hip.hpp).

Rows are views into one float32 array, passed as host buffers: a refused
layout returns DSP_ERR_INVALID with the call's text before any device is
looked at; an accepted one gets as far as the device (DSP_ERR_NO_DEVICE
without a GPU, DSP_OK with one, where it computes on memory the test owns).
Lengths are the smallest the plans allow: rows of 64 samples, n = 1024.
"""
import collections
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


# ---------------------------------------------------------------------------
# The 8192-point grid calls (dsp_welch, dsp_stft, dsp_istft, dsp_pvoc,
# dsp_time_stretch) and dsp_decay.  One rule for all of them: no output row may
# overlap an input row, a row of another output set, or a row of its own set.
# A call is its row sets in argument order; the cases below are made from the
# sets, one for every pair the rule names.
# Sizes: one frame (dsp_welch) or two frames at hop 4096 of the 8192-point
# grid; spectrum rows at a leading dimension past 2 K, so that a row ends at
# its last frame's 2 K and not at F ld; dsp_decay on rows of 64 samples of one
# high octave (n = 1024, three entries per output row).
# ---------------------------------------------------------------------------
NG, K2, HOP = 8192, 2 * 4097, 4096
LG = NG + HOP       # two frames
LD = K2 + 6         # floats from a frame to the next: six the call leaves alone after each 2 K
SPAN = LD + K2      # a two-frame spectrum row
DL, DHOPS, DBANDS = 64, 3, (1, 3, 3)

# rows, floats per row, the alignment its call asks for (in floats), written by the call
Set = collections.namedtuple("Set", "name rows floats align out")
_IN2, _SXX = Set("in", 2, NG, 1, False), Set("sxx", 2, K2, 2, True)
_DIN, _PEAK, _ONSET = Set("in", 2, DL, 1, False), Set("peak", 1, 2, 1, True), Set("onset", 1, 4, 2, True)
_ENERGY, _MOMENT = Set("energy", 2, 2 * DHOPS, 2, True), Set("moment", 2, 2 * DHOPS, 2, True)
GRID = {
    "welch": [_IN2, _SXX],
    "welch-ref": [_IN2, Set("ref", 1, NG, 1, False), _SXX, Set("srr", 1, K2, 2, True), Set("sxy", 2, 2 * K2, 2, True)],
    "stft": [Set("in", 2, LG, 1, False), Set("spec", 2, SPAN, 2, True)],
    "istft": [Set("spec", 2, SPAN, 2, False), Set("out", 2, LG, 1, True)],
    "pvoc": [Set("spec_in", 2, SPAN, 2, False), Set("spec_out", 2, SPAN, 2, True)],
    "time_stretch": [Set("in", 2, LG, 1, False), Set("out", 2, LG, 1, True)],
    "decay": [_DIN, _PEAK, _ONSET, _ENERGY],
    "decay-moment": [_DIN, _PEAK, _ONSET, _ENERGY, _MOMENT],
}
GRID_TEXT = {c: b"dsp_%s: an output row overlaps an input row or another output row" % c.encode()
             for c in ("welch", "stft", "istft", "pvoc", "time_stretch", "decay")}


def _packed(sets):
    """Every row right behind the one before it: all of them touch, none overlap."""
    at, o = {}, 0
    for s in sets:
        assert o % s.align == 0 and s.floats % s.align == 0
        at[s.name] = [o + r * s.floats for r in range(s.rows)]
        o += s.rows * s.floats
    return at, o


def _free(sets):
    """An even offset with the longest row's length free on either side, past the packed rows."""
    longest = max(s.floats for s in sets)
    return (_packed(sets)[1] + longest + 2) & ~1, longest


def _grid_cases():
    """(call, layout, refused) by id.  For sets a and b, the last row of each moves to the
    free space: b's to `free`, a's so that it ends `g` floats into b's (start), begins `g`
    floats before b's end (end), begins where b's does (same), or touches it on either side
    (before, after); g is one float, or two where both rows must be 8-byte aligned.  For b
    alone its two rows take those places."""
    cases = {}
    for call, sets in GRID.items():
        base, free = _packed(sets)[0], _free(sets)[0]
        cases[f"{call}:packed"] = (call, base, False)
        for j, b in enumerate(sets):
            if not b.out:
                continue
            for i, a in enumerate(sets):
                if a.out and i > j:
                    continue  # (each pair of output sets once)
                fix, mov = (a, b) if a.align > b.align else (b, a)
                g = mov.align
                places = {"start": free - mov.floats + g, "end": free + fix.floats - g, "same": free,
                          "before": free - mov.floats, "after": free + fix.floats}
                if a is b:
                    if b.rows < 2:
                        continue
                    del places["start"], places["before"]
                for where, o in places.items():
                    at = {k: list(v) for k, v in base.items()}
                    if a is b:
                        at[b.name][-2] = free
                    at[fix.name][-1] = free
                    at[mov.name][-1] = o
                    assert o % mov.align == 0
                    cases[f"{call}:{a.name}/{b.name}:{where}"] = (call, at, where in ("start", "end", "same"))
    return cases


GRID_CASES = _grid_cases()


def _table(buf, offsets, ptr):
    t = (ptr * len(offsets))()
    for i, o in enumerate(offsets):
        t[i] = C.cast(C.c_void_p(buf.ctypes.data + 4 * o), ptr)
    return t


def _grid_call(buf, call, at):
    lib, ex, L = d.lib(), _ex(), _lib
    assert buf.ctypes.data % 8 == 0
    fl = lambda name: _table(buf, at[name], L.FP)  # noqa: E731
    db = lambda name: _table(buf, at[name], L.DP) if name in at else None  # noqa: E731
    one = lambda name, ptr: _table(buf, at[name], ptr)[0] if name in at else None  # noqa: E731
    u64 = lambda: C.c_uint64(0)  # noqa: E731
    kind = call.split("-")[0]
    if kind == "welch":
        sp = L.dsp_welch_spec(NG, HOP, L.DSP_WIN_HANN)
        return lib.dsp_welch(fl("in"), 2, NG, one("ref", L.FP), db("sxx"), one("srr", L.DP), db("sxy"), C.byref(sp),
                             C.byref(ex))
    if kind == "stft":
        sp, frames = L.dsp_stft_spec(NG, HOP, L.DSP_WIN_HANN), u64()
        assert lib.dsp_stft_plan(LG, 2, C.byref(sp), C.byref(frames), None, None) == 0 and frames.value == 2
        return lib.dsp_stft(fl("in"), 2, LG, fl("spec"), LD, C.byref(sp), C.byref(ex))
    if kind == "istft":
        sp, full = L.dsp_istft_spec(NG, HOP, L.DSP_WIN_HANN, 1e-10), u64()
        assert lib.dsp_istft_plan(2, 2, C.byref(sp), C.byref(full), None, None, None) == 0 and full.value == LG
        return lib.dsp_istft(fl("spec"), 2, 2, LD, fl("out"), LG, C.byref(sp), C.byref(ex))
    if kind == "pvoc":
        sp, frames = L.dsp_pvoc_spec(1.0), u64()
        assert lib.dsp_pvoc_plan(2, 2, C.byref(sp), C.byref(frames), None, None) == 0 and frames.value == 2
        return lib.dsp_pvoc(fl("spec_in"), 2, 2, LD, fl("spec_out"), LD, C.byref(sp), C.byref(ex))
    if kind == "time_stretch":
        sp, full = L.dsp_stretch_spec(1.0, NG, HOP, L.DSP_WIN_HANN, 1e-10), u64()
        assert lib.dsp_time_stretch_plan(LG, 2, C.byref(sp), None, None, C.byref(full), None, None) == 0
        assert full.value == LG
        return lib.dsp_time_stretch(fl("in"), 2, LG, fl("out"), LG, C.byref(sp), C.byref(ex))
    assert kind == "decay"
    sp, bands, hops = L.dsp_decay_spec(*DBANDS), C.c_uint32(0), u64()
    assert lib.dsp_decay_plan(DL, 2, SR, C.byref(sp), None, None, None, C.byref(bands), C.byref(hops), None, None) == 0
    assert bands.value == 1 and hops.value == DHOPS
    return lib.dsp_decay(fl("in"), 2, DL, SR, C.byref(sp), one("peak", L.FP), one("onset", C.POINTER(C.c_uint64)),
                         db("energy"), db("moment"), C.byref(ex))


def _grid_check(call, at, refused):
    free, longest = _free(GRID[call])
    buf = np.random.default_rng(7).uniform(-0.5, 0.5, free + 2 * longest + 8).astype(np.float32)
    for s in GRID[call]:
        assert all(0 <= o and o + s.floats <= buf.size for o in at[s.name])
    before = buf.copy()
    st = _grid_call(buf, call, at)
    if refused:
        assert st == _lib.DSP_ERR_INVALID, (st, d.lib().dsp_last_error())
        assert d.lib().dsp_last_error() == GRID_TEXT[call.split("-")[0]]
        assert np.array_equal(buf.view(np.uint32), before.view(np.uint32))
    else:  # as far as the device
        assert st in (_lib.DSP_OK, _lib.DSP_ERR_NO_DEVICE), (st, d.lib().dsp_last_error())


@pytest.mark.parametrize("case", sorted(GRID_CASES))
def test_grid_and_decay_rows(case):
    _grid_check(*GRID_CASES[case])


def test_grid_cases_cover_every_pair_the_rule_names():
    """welch with ref: 3 x 2 output-input pairs, 3 output-output pairs, 2 sets of two rows;
    decay with moment: 4 + 6 and 2.  Five places a pair, three a set."""
    ids = [k for k in GRID_CASES if k.startswith("welch-ref:") and k != "welch-ref:packed"]
    assert len(ids) == 5 * (6 + 3) + 3 * 2
    ids = [k for k in GRID_CASES if k.startswith("decay-moment:") and k != "decay-moment:packed"]
    assert len(ids) == 5 * (4 + 6) + 3 * 2
    assert sum(r for _, _, r in GRID_CASES.values()) > sum(not r for _, _, r in GRID_CASES.values()) > len(GRID)


@pytest.mark.parametrize("call,a,b", [("stft", "spec", "spec"), ("pvoc", "spec_out", "spec_out"),
                                      ("pvoc", "spec_in", "spec_out"), ("istft", "spec", "out")])
def test_a_spectrum_row_ends_at_its_last_frames_2K(call, a, b):
    """The neighbour of a two-frame row at ld > 2 K: refused where it starts inside the last
    frame's [0, 2 K), accepted from the last frame's 2 K on -- before the row's F ld."""
    assert SPAN < 2 * LD
    base, free = _packed(GRID[call])[0], _free(GRID[call])[0]
    g = 2 if b.startswith("spec") else 1
    for o, refused in ((LD, True), (SPAN - g, True), (SPAN, False)):
        at = {k: list(v) for k, v in base.items()}
        if a == b:
            at[a] = [free, free + o]
        else:
            at[a][-1], at[b][-1] = free, free + o
        _grid_check(call, at, refused)
