"""Positions past 2^32: sample offsets, cursors, row lengths, frame indices
and byte offsets that do not fit 32 bits, through every call that forms one.

Tier 1  sample offsets of 2^32 - 2B .. 2^53 - 4B on small buffers.  The
        per-sample maps see a position only through (O + i) mod B, so the
        expectation is the oracle's render at offset 0 (bigutil.ramp_slice).
        dsp_exec.sample_offset must be a multiple of B (dspbench.h), so at
        B = 100 and B = 384 each listed offset is also run moved up to the
        next multiple of B (bigutil.accepted_offsets), and every listed offset
        that is no multiple of B must be refused with DSP_ERR_INVALID.
Tier 2  rows whose byte offset passes 4 GiB (allocations of 5-9 GiB).
Tier 3  one row of 2^32 + 12,345 floats: sample indices past 2^32; and
        magnitude matrices of more than 2^32 floats, where a row offset f * ld
        formed in 32 bits wraps.

Every expectation is the oracle's, a closed form (bigutil, stftutil, numpy
restatements of the test plugins) or torch arithmetic on the device; bit
equality with a second call of the library is only ever an extra assertion.
Nothing large is copied to the host: comparisons run on the device in slices.

Constants, none of them new: PEAK_REL_TOL and peak_rel_err are
test_gpu_parity.py's; SENTINEL is rowsutil.py's; the impulse bound is
stftutil.check_impulses'.

A test skips only when torch.cuda.mem_get_info() reports less free memory
than its stated need (the *_GIB constant beside it) plus 4 GiB.
"""
import contextlib
import ctypes as C
import gc
import math
import os

import numpy as np
import pytest

import bigutil as bu
import dspbench as d
import dspbench._lib as L
import rowsutil as ru
import stftutil as su
from dspbench.api import last_result
from test_gpu_parity import PEAK_REL_TOL, peak_rel_err
from test_gpu_proof import blocks as plugin_blocks, semantics as plugin_semantics
from test_gpu_specialize import CLIP_SRC, RAMP_F32_SRC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N = 8192
K = 4097
SR = 48000.0
GIB = 1 << 30
HANN = d.DSP_WIN_HANN
S = int(ru.SENTINEL)
# include/dspbench/dspbench.h
DSP_RESULT_SPECTRUM_CACHE = 0x10
DSP_DEBUG_SPECTRUM_CACHE = 4
DSP_DEBUG_ROW_RUN = 5
REUSE = L.DSP_RESULT_FRAME_REUSE
BOTH = REUSE | DSP_RESULT_SPECTRUM_CACHE

BIG_N = bu.P32 + 12_345        # Tier 3's row
F_BIG = 262_400                # Tier 2's frame count at N = 8192, H = 128

PLUGINS = {
    # name: (plugin, the oracle's restated plugin, ignores its input)
    "gain_test": (lambda: d.Plugin.gain_test(0.2), "gain_test", False),
    "IR_test": (lambda: d.Plugin.ir_test(0.9, 0.002), "IR_test", True),
    "static_gain": (lambda: d.Plugin.static_gain(0.1), "static_gain_plugin", False),
    "no_op": (lambda: d.Plugin.no_op(), "no_op", False),
}


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def need(torch, gib):
    """The one reason to skip: less free device memory than the need + 4 GiB."""
    release(torch)
    free = torch.cuda.mem_get_info()[0]
    if free < (gib + 4) * GIB:
        pytest.skip(f"{free / GIB:.1f} GiB free on the device, the test needs {gib} + 4 GiB")


def release(torch):
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _set(what, value):
    L.check(L.lib().dsp_debug_set(what, value), "dsp_debug_set")


@contextlib.contextmanager
def hooks(cache=2, row_run=0, frame_run=0):
    """cache 2: the spectrum row off; 1: forced wherever it is valid (the
    store-only rows launch, row_run frames per wave); frame_run: frames per wave
    of the reuse launch (test_gpu_spectrum_cache.py, test_gpu_rows_pacing.py)."""
    _set(DSP_DEBUG_SPECTRUM_CACHE, cache)
    _set(DSP_DEBUG_ROW_RUN, row_run)
    _set(L.DSP_DEBUG_FRAME_RUN, frame_run)
    try:
        yield
    finally:
        _set(DSP_DEBUG_SPECTRUM_CACHE, 0)
        _set(DSP_DEBUG_ROW_RUN, 0)
        _set(L.DSP_DEBUG_FRAME_RUN, 0)


def refused(call, match):
    with pytest.raises(d.DspError, match=match) as e:
        call()
    assert e.value.status == L.DSP_ERR_INVALID


def rnd(shape, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=shape).astype(np.float32)


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def oracle_render(oracle, kind, x, Cn, B, L_):
    """The oracle's render at offset 0: of the file for the gain kinds, of a
    file B samples longer (no input: the ramp ignores it) for IR_test."""
    _, oname, ramp = PLUGINS[kind]
    plug = oracle.restated_plugin(oname)
    if ramp:
        return oracle.render_offline([], Cn, B, SR, plug, L=L_ + B)
    return oracle.render_offline([x[c] for c in range(x.shape[0])], Cn, B, SR, plug, L=L_)


def expect_at(kind, ref, O, B, n):
    return bu.ramp_slice(ref, O, B, n) if PLUGINS[kind][2] else ref[:, :n]


def ramp_tile(torch, oracle, B):
    return dev(torch, oracle.ir_ramp_reference(0.9, 0.002, B))


def sentinel_rows(torch, shape):
    return torch.full(shape, S, dtype=torch.int32, device="cuda").view(torch.float32)


def sentinel_counts(torch, mag, Kc, step=1 << 15):
    """(SENTINEL words left in columns [0, Kc), words changed in the pad
    columns [Kc, ld)) of mag [F, ld], counted on the device in slices."""
    w = mag.view(torch.int32)
    left = torch.zeros((), dtype=torch.int64, device="cuda")
    touched = torch.zeros((), dtype=torch.int64, device="cuda")
    for f0 in range(0, w.shape[0], step):
        blk = w[f0:f0 + step]
        left += (blk[:, :Kc] == S).sum()
        touched += (blk[:, Kc:] != S).sum()
    return int(left), int(touched)


def same_bits_dev(torch, a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def blocks_equal(torch, row, tile, step_blocks=1 << 19):
    """Every block of the 1-D row (a whole number of blocks) equals tile, bit for bit."""
    B = tile.shape[0]
    assert row.dim() == 1 and row.shape[0] % B == 0
    t = tile.view(torch.int32)[None]
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    for i0 in range(0, row.shape[0], step_blocks * B):
        blk = row[i0:i0 + step_blocks * B].view(torch.int32).view(-1, B)
        bad += (blk != t).sum()
    return int(bad) == 0


# ---------------------------------------------------------------------------
# Tier 1 -- positions past 2^32 on small buffers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", [512, 100, 384])
@pytest.mark.parametrize("kind", list(PLUGINS))
def test_t1_render_offline(torch_cuda, oracle, kind, B):
    """Aligned rows (the vector kernel, three tiles and a ragged one) and
    output rows one float off (the scalar kernel), rowsutil guards intact."""
    torch = torch_cuda
    Cn, L_ = 2, 3 * 4096 + 4 * B + 37
    n = d.num_blocks(L_, B) * B
    x = rnd((Cn, L_), 11)
    ref = oracle_render(oracle, kind, x, Cn, B, L_)
    for layout in ("base", "out1"):
        ioff, ooff, sm = ru.LAYOUTS[layout]
        for name, O in bu.accepted_offsets(B):
            rin = ru.Rows(Cn, L_, off=ioff, stride_mod=sm, torch=torch).fill(x)
            rout = ru.Rows(Cn, n, off=ooff, stride_mod=sm, torch=torch)
            d.render_offline(rin.view, Cn, B, SR, PLUGINS[kind][0](), out=rout.view, sample_offset=O, L_file=L_)
            torch.cuda.synchronize()
            rout.check_output()
            assert ru.same_bits(rout.numpy(), np.ascontiguousarray(expect_at(kind, ref, O, B, n))), (layout, name)
    rin = ru.Rows(Cn, L_, torch=torch).fill(x)
    rout = ru.Rows(Cn, n, torch=torch)
    for O in bu.refused_offsets(B):
        refused(lambda: d.render_offline(rin.view, Cn, B, SR, PLUGINS[kind][0](), out=rout.view, sample_offset=O,
                                         L_file=L_), "multiple of B")
    torch.cuda.synchronize()
    rout.check_guards(0)  # a refused call writes nothing


@pytest.mark.parametrize("L_", [1000, 5000])
@pytest.mark.parametrize("B", [512, 100, 384])
@pytest.mark.parametrize("kind", ["gain_test", "IR_test"])
def test_t1_render_loop(torch_cuda, oracle, kind, B, L_):
    """A large sample_offset with a cursor three samples before the end of the
    file, four wraps: L = 1000 wraps by modulo inside every tile, L = 5000 by
    compare (render_wrap_vec_kernel), out1 the scalar wrap kernel."""
    torch = torch_cuda
    Cn, cursor = 2, L_ - 3
    nblocks = -(-4 * L_ // B) + 1
    n = nblocks * B
    x = rnd((Cn, L_), 71)
    plug = oracle.restated_plugin(PLUGINS[kind][1])
    ref, _ = oracle.render_loop([x[0], x[1]], Cn, B, nblocks + 1, SR, plug, cursor=cursor)
    _, ref_cur = oracle.render_loop([x[0], x[1]], Cn, B, nblocks, SR, plug, cursor=cursor)
    assert ref_cur == (cursor + n) % L_
    if not PLUGINS[kind][2]:  # the oracle's loop is the closed form's index map
        g = np.float32(0.2)
        assert np.array_equal(ref[:, :n], x[:, bu.loop_index(cursor, 0, n, L_)] * g)
    for layout in ("base", "out1"):
        ioff, ooff, sm = ru.LAYOUTS[layout]
        for name, O in bu.accepted_offsets(B):
            rin = ru.Rows(Cn, L_, off=ioff, stride_mod=sm, torch=torch).fill(x)
            rout = ru.Rows(Cn, n, off=ooff, stride_mod=sm, torch=torch)
            _, cur = d.render_loop(rin.view, Cn, B, nblocks, SR, PLUGINS[kind][0](), cursor=cursor, out=rout.view,
                                   sample_offset=O)
            torch.cuda.synchronize()
            assert cur == ref_cur
            rout.check_output()
            assert ru.same_bits(rout.numpy(), np.ascontiguousarray(expect_at(kind, ref, O, B, n))), (layout, name)
    for O in bu.refused_offsets(B):
        refused(lambda: d.render_loop(dev(torch, x), Cn, B, nblocks, SR, PLUGINS[kind][0](), cursor=cursor,
                                      sample_offset=O), "multiple of B")


def stft_call(torch, plugin, x, Cn, B, L_, H, ld, O, phase=0):
    """dsp_render_stft on SENTINEL rows with guards: (out Rows, mag Rows, result bits, F)."""
    Lr = d.num_blocks(L_, B) * B
    F = d.stft_frames(Lr, N, H)
    out = ru.Rows(Cn, Lr, off=0, torch=torch)
    mag = ru.Rows(Cn, F * ld, off=phase, torch=torch)
    file = torch.zeros((Cn, L_ + (L_ & 1)), device="cuda")
    if x is not None:
        file[:, :L_] = dev(torch, x)
    d.render_stft(file, Cn, B, SR, plugin, H=H, window=HANN, ld=ld, out=out.view, mag=mag.frames(F, ld),
                  sample_offset=O, L_file=L_)
    res = last_result()
    torch.cuda.synchronize()
    out.check_output()
    mag.check_output(F * ld, K, ld)
    return out, mag, res, F


def mags_of(mag, Cn, F, ld):
    return mag.numpy(F * ld).reshape(Cn, F, ld)[:, :, :K]


def oracle_mags(oracle, want, H):
    return [oracle.np_stft_mag(want[c], N, H, HANN, K) for c in range(want.shape[0])]


def check_against_oracle(got_out, got_mag, want, mref, what):
    assert ru.same_bits(got_out, np.ascontiguousarray(want)), what
    for c in range(want.shape[0]):
        err = peak_rel_err(got_mag[c], mref[c])
        assert err <= PEAK_REL_TOL, (what, c, err)


@pytest.mark.parametrize("ld", [4097, 4099])
@pytest.mark.parametrize("H", [4096, 1000])
@pytest.mark.parametrize("B", [512, 100, 384, 4096])
@pytest.mark.parametrize("kind", ["gain_test", "IR_test"])
def test_t1_render_stft(torch_cuda, oracle, kind, B, H, ld):
    """The plain launch: H = 4096 is the fused kernel (the periodic frame at
    B = 512, the table gather with its 64-bit `% B` at B = 100 and 384, no
    periodic frame at B = 4096), H = 1000 the render and the memory STFT; a
    ragged file whose last block no frame owns."""
    torch = torch_cuda
    Cn, L_ = 2, 4 * 4096 + N + 17
    n = d.num_blocks(L_, B) * B
    x = rnd((Cn, L_), 31)
    ref = oracle_render(oracle, kind, x, Cn, B, L_)
    want = expect_at(kind, ref, 0, B, n)
    mref = oracle_mags(oracle, want, H)
    with hooks(cache=2):
        for name, O in bu.accepted_offsets(B):
            assert np.array_equal(expect_at(kind, ref, O, B, n), want)  # (every accepted offset has phase 0)
            out, mag, res, F = stft_call(torch, PLUGINS[kind][0](), x, Cn, B, L_, H, ld, O, phase=1)
            assert F == mref[0].shape[0] and res & BOTH == 0
            check_against_oracle(out.numpy(), mags_of(mag, Cn, F, ld), want, mref, (name, O))
        for O in bu.refused_offsets(B):
            refused(lambda: stft_call(torch, PLUGINS[kind][0](), x, Cn, B, L_, H, ld, O), "multiple of B")


@pytest.mark.parametrize("B,H", [(512, 4096), (128, 4096), (2048, 4096), (512, 1024)])
def test_t1_render_stft_launch_variants(torch_cuda, oracle, B, H):
    """IR_test with H % B == 0 at large offsets: one FFT per frame
    (DSP_EXEC_EVERY_FRAME), the plain launch, the frame-reuse launch
    (DSP_DEBUG_FRAME_RUN), the cached spectrum row and the store-only rows
    launch at two run lengths.  The file ends 17 samples past the last frame,
    so the tail waves render the blocks no frame owns.  The every-frame call is
    held to the oracle; the others equal it bit for bit, as
    test_gpu_spectrum_cache.py and test_gpu_frame_reuse.py assert at offset 0."""
    torch = torch_cuda
    Cn, F0 = 2, 9
    L_ = (F0 - 1) * H + N + 17
    n = d.num_blocks(L_, B) * B
    ref = oracle_render(oracle, "IR_test", None, Cn, B, L_)
    want = expect_at("IR_test", ref, 0, B, n)
    mref = oracle_mags(oracle, want, H)
    cached, every = d.Plugin.ir_test(0.9, 0.002), d.Plugin.ir_test(0.9, 0.002, every_frame=True)
    variants = [("plain", cached, dict(cache=2), 0), ("reuse", cached, dict(cache=2, frame_run=4), REUSE),
                ("row", cached, dict(cache=1), BOTH), ("rows2", cached, dict(cache=1, row_run=2), BOTH)]
    for ld in (4097, 4099):
        for name, O in bu.accepted_offsets(B):
            with hooks(cache=2):
                eo, em, res, F = stft_call(torch, every, None, Cn, B, L_, H, ld, O, phase=ld & 3)
            assert res & BOTH == 0 and F == F0
            eo, em = eo.numpy(), mags_of(em, Cn, F, ld)
            check_against_oracle(eo, em, want, mref, (name, O, ld))
            for vname, plug, hk, bits in variants:
                with hooks(**hk):
                    out, mag, res, _ = stft_call(torch, plug, None, Cn, B, L_, H, ld, O, phase=ld & 3)
                assert res & BOTH == bits, (vname, hex(res), name)
                assert ru.same_bits(out.numpy(), eo) and ru.same_bits(mags_of(mag, Cn, F, ld), em), (vname, name, ld)


@pytest.fixture(scope="module")
def modules(torch_cuda):
    """GENERIC plugins compiled from source: a float ramp (the table class,
    test_gpu_specialize.RAMP_F32_SRC), tests/plugins/fade_in.cpp (the gain-table
    class) and a clipping gain (no class: the callback on every block,
    test_gpu_specialize.CLIP_SRC)."""
    with open(os.path.join(HERE, "plugins", "fade_in.cpp")) as f:
        fade = f.read()
    out = {}
    for name, src, cls in (("ramp_f32", RAMP_F32_SRC, "table"), ("fade_in", fade, "gain_table"),
                           ("clip", CLIP_SRC, "callback")):
        mod = d.module.Module(d.module.compile_source(src, f"{name}.cpp"))
        params = mod.default_parameters()
        mod.initialize_state(params, 2, SR)
        out[name] = (mod, params, cls)
    return out


def generic_semantics(name, x, Cn, B, params):
    """The callback on every block of the file, in numpy float32."""
    xb = plugin_blocks(x, Cn, B)
    if name == "fade_in":
        return plugin_semantics("fade_in", xb, params)
    if name == "clip":  # out = x > 5 ? 0 : x * g
        g = np.frombuffer(params[:4], np.float32)[0]
        return np.where(xb > np.float32(5), np.float32(0), xb * g).astype(np.float32).reshape(Cn, -1)
    g, st = np.frombuffer(params[:8], np.float32)  # ramp_f32: a float recurrence restarted at every block
    tile = np.empty(B, np.float32)
    for s in range(B):
        tile[s] = g
        g = np.float32(g - st)
    return np.tile(tile, (Cn, xb.shape[1]))


@pytest.mark.parametrize("B", [512, 100, 384])
@pytest.mark.parametrize("name", ["ramp_f32", "fade_in", "clip"])
def test_t1_generic_modules(torch_cuda, oracle, modules, name, B):
    """GENERIC plugins at every accepted offset: rendered by their block class
    and by the callback on every block, both equal to the callback's numpy
    restatement; render + STFT (the fused kernel's table and gain-table frames
    for the classes) held to the oracle's float64 STFT of that render."""
    torch = torch_cuda
    mod, params, cls = modules[name]
    Cn, L_ = 2, 4 * 4096 + N + 17
    n = d.num_blocks(L_, B) * B
    assert mod.block_class(params, Cn, B, SR)[0] == cls
    x = rnd((Cn, L_), 5, -8.0, 8.0)
    want = generic_semantics(name, x, Cn, B, params)
    assert want.shape == (Cn, n)
    mref = oracle_mags(oracle, want, 4096)
    xg = dev(torch, x)
    for oname, O in bu.accepted_offsets(B):
        for spec in (True, False):
            got = d.render_offline(xg, Cn, B, SR, mod.plugin(params, name, specialize=spec), sample_offset=O)
            assert ru.same_bits(got.cpu().numpy(), want), (oname, spec)
        out, mag, _, F = stft_call(torch, mod.plugin(params, name), x, Cn, B, L_, 4096, 4099, O, phase=1)
        check_against_oracle(out.numpy(), mags_of(mag, Cn, F, 4099), want, mref, (oname, O))
    for O in bu.refused_offsets(B):
        refused(lambda: d.render_offline(xg, Cn, B, SR, mod.plugin(params, name), sample_offset=O), "multiple of B")


@pytest.mark.parametrize("B", [512, 100])
@pytest.mark.parametrize("kind", ["gain_test", "IR_test"])
def test_t1_render_stft_host(torch_cuda, oracle, kind, B):
    """The chunked host driver hands chunk c sample_offset + c.start: ten
    chunks of 3 * 4096 starting five chunks below 2^32, so the chunk offsets
    straddle it."""
    chunk = 3 * 4096
    O = bu.aligned_up(bu.P32 - 5 * chunk, B)
    assert O < bu.P32 < O + 6 * chunk
    Cn, L_ = 2, 10 * chunk + 777
    n = d.num_blocks(L_, B) * B
    x = rnd((Cn, L_), 41)
    ref = oracle_render(oracle, kind, x, Cn, B, L_)
    want = expect_at(kind, ref, O, B, n)
    out, mag = d.render_stft_host(x, Cn, B, SR, PLUGINS[kind][0](), chunk=chunk, sample_offset=O)
    check_against_oracle(out, mag, want, oracle_mags(oracle, want, 4096), (kind, B))
    for bad in bu.UNALIGNED:
        refused(lambda: d.render_stft_host(x, Cn, B, SR, PLUGINS[kind][0](), chunk=chunk, sample_offset=bad),
                "multiple of B")


def test_t1_whole_file_plugins_refuse_an_offset(torch_cuda):
    """FIR, CONV and BIQUAD carry state across blocks: whole files only
    (dspbench.h), at a large offset as at a small one."""
    torch = torch_cuda
    x = torch.zeros((1, 4096), device="cuda")
    out = sentinel_rows(torch, (1, 4096))
    taps = rnd((33,), 3) * 0.1
    for plug in (d.Plugin.fir(taps), d.Plugin.fir(taps, direct=True), d.Plugin.conv(taps),
                 d.Plugin.biquad(d.Plugin.biquad_lowpass_coefficients())):
        for O in (512, bu.P32, bu.P40 + 512):
            refused(lambda: d.render_offline(x, 1, 512, SR, plug, out=out, sample_offset=O), "whole files only")
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == S).all())


# ---------------------------------------------------------------------------
# Tier 2 -- byte offsets past 4 GiB
# ---------------------------------------------------------------------------
STFT_GIB = 7  # a 4.3 GB magnitude matrix, a 134 MB signal, slice temporaries


def stft_rows_past_4gib(torch, oracle, Nn, H, F, lds, pixels, line_bytes=bu.P32, Kn=None):
    Kn = Nn // 2 + 1 if Kn is None else Kn
    L_ = Nn + H * (F - 1)
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand((1, L_), device="cuda", generator=g) * 2 - 1
    for ld in lds:
        assert F * ld * 4 > line_bytes + (1 << 20)
        mag = sentinel_rows(torch, (1, F, ld))
        got = d.stft_magnitude(x, N=Nn, H=H, window=HANN, K=Kn, ld=ld, out=mag)
        assert got.shape == (1, F, Kn)
        line = bu.first_row_past(line_bytes, ld)
        assert 308 < line < F - 308
        for f0, f1 in ((0, 300), (F - 300, F), (line - 8, line + 8)):
            seg = x[:, f0 * H:(f1 - 1) * H + Nn]
            rows = mag[0, f0:f1, :Kn]
            small = d.stft_magnitude(seg, N=Nn, H=H, window=HANN, K=Kn)
            assert same_bits_dev(torch, small[0], rows), (ld, f0)
            ref = oracle.np_stft_mag(seg[0].cpu().numpy(), Nn, H, HANN, Kn)
            err = peak_rel_err(rows.cpu().numpy(), ref)
            assert err <= PEAK_REL_TOL, (ld, f0, err)
        left, touched = sentinel_counts(torch, mag[0], Kn)
        assert left == 0, f"{left} magnitudes never written (ld = {ld})"
        assert touched == 0, f"{touched} pad words written (ld = {ld})"
        if pixels:  # the overview of this matrix: each pixel row is the maximum over its frames
            view = mag[0][:, :Kn]
            over = d.spectrogram_decimate(view, pixels)
            want = torch.stack([torch.amax(view[bu.pixel_first(p, pixels, F):bu.pixel_first(p + 1, pixels, F)], dim=0)
                                for p in range(pixels)])
            assert bool((view[-300:] >= 0).all()) and bool(torch.isfinite(want).all())
            assert torch.equal(over, want), ld
            del over, want, view
        del mag, got, rows, small
        release(torch)


def test_t2_stft8192_rows_past_4gib(torch_cuda, oracle):
    """stft_magnitude, N = 8192, C = 1, H = 128, F = 262,400 (33.6 M samples of
    noise), ld = 4097 and 4100: rows from f = 262,081 on start past 2^32 bytes.
    The first 300 rows, the last 300 and the 16 around the 4 GiB line equal the
    oracle's np_stft_mag of their slice (PEAK_REL_TOL, test_gpu_parity.py) and,
    bit for bit, a small call on that slice; no SENTINEL (rowsutil.py) is left
    in columns [0, K) and the pad columns are untouched.  Then
    spectrogram_decimate of the matrix, P = 1920: each output row is torch.amax
    over its frames [ceil(p F / P), ceil((p + 1) F / P)) -- exact, the
    magnitudes being finite and non-negative."""
    need(torch_cuda, STFT_GIB)
    assert bu.first_row_past(bu.P32, 4097) == 262_081
    stft_rows_past_4gib(torch_cuda, oracle, 8192, 128, F_BIG, (4097, 4100), 1920)


def test_t2_stft1024_rows_past_4gib(torch_cuda, oracle):
    """The same for the generic kernel: N = 1024, H = 16, F = 2,093,600
    (F * 513 * 4 > 2^32 + 2^20), ld = 513 and 516."""
    need(torch_cuda, STFT_GIB)
    stft_rows_past_4gib(torch_cuda, oracle, 1024, 16, 2_093_600, (513, 516), 0)


F_ELEMS = 1_048_900  # frames of 4097 floats: rows from 1,048,321 on start past 2^32 floats (16 GiB)


@pytest.mark.parametrize("B,F_min,ld", [(512, F_BIG, 4100), (128, F_BIG, 4100), (128, F_ELEMS, 4097)])
def test_t2_render_stft_fused_rows_past_4gib(torch_cuda, oracle, B, F_min, ld):
    """render_stft with IR_test, H = 128, at least 262,400 frames (rows past
    4 GiB) and at least 1,048,900 (rows past 2^32 floats: a row offset formed in
    32 bits wraps there, not at 4 GiB), at sample_offset 2^32.  B = 128 (H % B == 0) runs the plain, the frame-reuse
    and the store-only rows launch; B = 512 (every fourth frame the same) has
    no reusable frame and keeps the plain launch whatever the hooks ask.
    Every row equals the row of its phase in the first period (compared on
    the device), the first period is held to the oracle and equals a small
    DSP_EXEC_EVERY_FRAME call bit for bit, no SENTINEL is left and no pad word
    written, and the render is the oracle's ramp in every block."""
    torch = torch_cuda
    need(torch, F_min * ld * 4 // GIB + 3)  # the magnitude matrix, the render, slice temporaries
    H, O = 128, bu.P32
    L_ = N + H * (F_min - 1) + 17
    Lr = d.num_blocks(L_, B) * B
    F = d.stft_frames(Lr, N, H)
    per = math.lcm(B, H) // H
    assert F >= F_min and Lr > F * H and F * ld * 4 > bu.P32 + (1 << 20)
    assert F_min < F_ELEMS or F * ld > bu.P32 + (1 << 20)
    tile = ramp_tile(torch, oracle, B)
    first = np.tile(tile.cpu().numpy(), (N + per * H) // B + 1)[:N + (per - 1) * H]
    mref = oracle.np_stft_mag(first, N, H, HANN, K)
    assert mref.shape[0] == per
    with hooks(cache=2):
        _, sm, _, sF = stft_call(torch, d.Plugin.ir_test(0.9, 0.002, every_frame=True), None, 1, B,
                                 N + (per + 2) * H, H, K, O)
    small = dev(torch, mags_of(sm, 1, sF, K)[0, :per])
    reusable = H % B == 0
    # (every_frame, hooks, result bits): one FFT per frame; the frame-reuse launch (a call this long takes it
    # by itself where it is valid, and a forced run does); the cached row's store-only launch
    variants = [(True, dict(cache=2), 0), (False, dict(cache=2, frame_run=4), REUSE if reusable else 0),
                (False, dict(cache=1), BOTH if reusable else 0)]
    for every, hk, bits in variants:
        out = sentinel_rows(torch, (1, Lr))
        mag = sentinel_rows(torch, (1, F, ld))
        with hooks(**hk):
            d.render_stft(None, 1, B, SR, d.Plugin.ir_test(0.9, 0.002, every_frame=every), H=H, window=HANN, ld=ld,
                          out=out, mag=mag, sample_offset=O, L_file=L_)
            assert last_result() & BOTH == bits, (hk, hex(last_result()))
        w = mag[0].view(torch.int32)
        base = w[:per, :K]
        assert same_bits_dev(torch, mag[0, :per, :K].contiguous(), small), hk
        assert peak_rel_err(mag[0, :per, :K].cpu().numpy(), mref) <= PEAK_REL_TOL, hk
        bad = torch.zeros((), dtype=torch.int64, device="cuda")
        step = (1 << 15) // per * per
        for f0 in range(0, F, step):
            blk = w[f0:f0 + step, :K]
            whole = blk.shape[0] // per * per
            bad += (blk[:whole].unflatten(0, (-1, per)) != base[None]).sum()
            bad += (blk[whole:] != base[:blk.shape[0] - whole]).sum()
        assert int(bad) == 0, (hk, int(bad))
        left, touched = sentinel_counts(torch, mag[0], K)
        assert left == 0 and touched == 0, (hk, left, touched)
        assert blocks_equal(torch, out[0], tile), hk
        del out, mag, w, base, blk
        release(torch)


RENDER_GIB = 10  # input and output rows of 2^30 + 4099 floats, slice temporaries


@pytest.mark.parametrize("off", [0, 1])
def test_t2_render_offline_rows_past_4gib(torch_cuda, oracle, off):
    """render_offline, C = 1, L = 2^30 + 4099, output rows 16-byte aligned
    (the vector kernel) and one float off (the scalar kernel).  gain_test: the
    output is x * float32(0.2) by torch, bit for bit (the exactness
    test_gpu_parity.test_full_size_gain_render_10min establishes) and zero past
    the file.  IR_test at B = 100 with no input rows: every block is the
    oracle's block."""
    torch = torch_cuda
    need(torch, RENDER_GIB)
    L_ = (1 << 30) + 4099
    n512, n100 = d.num_blocks(L_, 512) * 512, d.num_blocks(L_, 100) * 100
    buf = sentinel_rows(torch, (max(n512, n100) + 8,))
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.rand((1, L_), device="cuda", generator=g) * 2 - 1
    out = buf[off:off + n512][None]
    assert (out.data_ptr() % 16 == 0) == (off == 0)
    d.render_offline(x, 1, 512, SR, d.Plugin.gain_test(0.2), out=out)
    gain = torch.tensor(0.2, dtype=torch.float32, device="cuda")
    for i0 in range(0, L_, 1 << 27):
        i1 = min(L_, i0 + (1 << 27))
        assert torch.equal(out[0, i0:i1], x[0, i0:i1] * gain), i0
    assert bool((out[0, L_:] == 0).all())
    assert bool((buf[:off].view(torch.int32) == S).all()) and bool((buf[off + n512:].view(torch.int32) == S).all())
    del x
    release(torch)
    buf.view(torch.int32).fill_(S)
    out = buf[off:off + n100][None]
    d.render_offline(None, 1, 100, SR, d.Plugin.ir_test(0.9, 0.002), out=out, L_file=L_)
    assert blocks_equal(torch, out[0], ramp_tile(torch, oracle, 100), step_blocks=1 << 21)
    assert bool((buf[:off].view(torch.int32) == S).all()) and bool((buf[off + n100:].view(torch.int32) == S).all())
    del out, buf
    release(torch)


LOOP_GIB = 7  # an output row of 2^30 + 1536 floats, index and gather temporaries


def test_t2_render_loop_past_4gib(torch_cuda):
    """render_loop, gain_test, nblocks * B = 2^30 + 512 * 3 from a
    480,000-sample file at cursor 1234: the output is x[(cursor + i) % L] * 0.2
    by torch indexing (bigutil.loop_index's rule, pinned against the oracle in
    test_large_positions_cpu.py), formed on the device in slices."""
    torch = torch_cuda
    need(torch, LOOP_GIB)
    B, L_, cursor = 512, 480_000, 1234
    nblocks = (1 << 21) + 3
    n = nblocks * B
    assert n == (1 << 30) + 512 * 3
    x = dev(torch, rnd((1, L_), 9))
    out = sentinel_rows(torch, (1, n))
    _, cur = d.render_loop(x, 1, B, nblocks, SR, d.Plugin.gain_test(0.2), cursor=cursor, out=out)
    assert cur == (cursor + n) % L_
    gain = torch.tensor(0.2, dtype=torch.float32, device="cuda")
    for i0 in range(0, n, 1 << 26):
        i1 = min(n, i0 + (1 << 26))
        idx = (torch.arange(i0, i1, dtype=torch.int64, device="cuda") + cursor) % L_
        assert torch.equal(out[0, i0:i1], x[0][idx] * gain), i0
        del idx
    del out
    release(torch)


def wav_info(bits, channels, frames, is_float=False):
    i = L.dsp_wav_info()
    i.format = 3 if is_float else 1
    i.channels = channels
    i.sample_rate = 48000
    i.bits_per_sample = bits
    i.block_align = channels * bits // 8
    i.frames = frames
    i.data_bytes = frames * i.block_align
    i.n_data_chunks = 1
    return i


def random_bytes(torch, nbytes):
    """A uint8 device payload of random bytes (the last nbytes % 8 are zero)."""
    payload = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(6)
    n8 = nbytes // 8
    step = 1 << 27
    words = payload[:n8 * 8].view(torch.int64)
    for i0 in range(0, n8, step):
        m = min(step, n8 - i0)
        words[i0:i0 + m] = torch.randint(-(1 << 63), (1 << 63) - 1, (m,), dtype=torch.int64, device="cuda",
                                         generator=g)
    return payload


def check_wav_windows(torch, oracle, payload, bits, channels, is_float, frame0s, frames=4099):
    ba = channels * bits // 8
    info = wav_info(bits, channels, payload.shape[0] // ba, is_float)
    for frame0 in frame0s:
        assert 0 <= frame0 and frame0 + frames <= info.frames
        got = d.wav.decode(payload, info, frame0, frames, device="cuda").cpu().numpy()
        raw = payload[frame0 * ba:(frame0 + frames) * ba].cpu().numpy()
        ref = oracle.deinterleave(oracle.pcm_to_float(raw, bits, is_float), channels)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (bits, channels, is_float, frame0)


WAV_DECODE_GIB = 14  # a 4.3 GB payload, 8.6 GB of decoded floats, slice temporaries


def test_t2_wav_decode_past_4gib(torch_cuda, oracle):
    """WAV decode from a random payload of 2^32 + 2^20 bytes as int16 stereo,
    int24 3-channel (the generic kernel) and float32 mono: windows of 4099
    frames below the 4 GiB byte line, straddling it, past it and at the end
    (even and odd frame0: every load width), bit for bit against
    oracle.pcm_to_float.  Then the whole payload as int16 mono equals
    payload.view(int16).float() * 2**-15 (the form wav.hip states and
    test_wav.py pins) on the device."""
    torch = torch_cuda
    need(torch, WAV_DECODE_GIB)
    nbytes = bu.P32 + (1 << 20)
    payload = random_bytes(torch, nbytes)
    for bits, channels, is_float in ((16, 2, False), (24, 3, False), (32, 1, True)):
        ba = channels * bits // 8
        line, frames = bu.P32 // ba, nbytes // ba
        check_wav_windows(torch, oracle, payload, bits, channels, is_float,
                          (line - 70_000, line - 70_001, line - 2000, line - 2001, line + 5000, line + 5003,
                           frames - 4099))
    # a multiple of four frames keeps every stereo output row 16-byte aligned: the tile kernel
    check_wav_windows(torch, oracle, payload, 16, 2, False, (bu.P32 // 4 - 2000, bu.P32 // 4 + 5002), frames=4100)
    info = wav_info(16, 1, nbytes // 2)
    got = d.wav.decode(payload, info, device="cuda")
    codes = payload.view(torch.int16)
    assert got.shape == (1, nbytes // 2)
    for i0 in range(0, nbytes // 2, 1 << 28):
        assert torch.equal(got[0, i0:i0 + (1 << 28)], codes[i0:i0 + (1 << 28)].float() * 2.0 ** -15), i0
    del got, codes, payload
    release(torch)


def wav_encode_into(torch, x, fmt, bits, buf):
    """dsp_wav_encode of x [C, n] into the device byte buffer buf."""
    ex = L.dsp_exec(torch.cuda.current_device(), L.DSP_EXEC_SYNC, C.c_void_p(torch.cuda.current_stream().cuda_stream), 0)
    ptrs = L.chan_table([x[c].data_ptr() for c in range(x.shape[0])])
    L.check(d.lib().dsp_wav_encode(ptrs, x.shape[0], x.shape[1], fmt, bits, C.c_void_p(buf.data_ptr()), C.byref(ex)),
            "dsp_wav_encode")


WAV_ENCODE_GIB = 10  # a row of 2^30 + 5 floats and its 4 GiB + 20 byte payload


def test_t2_wav_encode_past_4gib(torch_cuda, oracle):
    """WAV encode of a row of 2^30 + 5 samples (some clip).  float32: 4 GiB +
    20 bytes, a byte copy, compared as views.  int32 PCM: 2^20 sampled
    positions and the last 4099 against oracle.float_to_pcm.  0xA5 guard bytes
    after the payload stay intact."""
    torch = torch_cuda
    need(torch, WAV_ENCODE_GIB)
    n = (1 << 30) + 5
    g = torch.Generator(device="cuda").manual_seed(8)
    x = torch.rand((1, n), device="cuda", generator=g) * 2.2 - 1.1
    nbytes = 4 * n
    assert nbytes == bu.P32 + 20
    buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    wav_encode_into(torch, x, 3, 32, buf)
    assert torch.equal(buf[:nbytes].view(torch.int32), x[0].view(torch.int32))
    assert bool((buf[nbytes:] == 0xA5).all())
    buf.fill_(0xA5)
    wav_encode_into(torch, x, 1, 32, buf)
    idx = torch.cat([torch.randint(0, n, (1 << 20,), device="cuda", generator=g),
                     torch.arange(n - 4099, n, device="cuda")])
    want = oracle.float_to_pcm(x[0][idx].cpu().numpy(), 32).view(np.int32)
    assert np.array_equal(buf[:nbytes].view(torch.int32)[idx].cpu().numpy(), want)
    assert int(idx.max()) == n - 1 and int((idx >= (1 << 29)).sum()) > 1 << 18  # positions past 2 GiB of payload
    assert bool((buf[nbytes:] == 0xA5).all())
    del x, buf, idx
    release(torch)


# ---------------------------------------------------------------------------
# Tier 3 -- one row of 2^32 + 12,345 floats
# ---------------------------------------------------------------------------
def planted_row(torch, vals):
    x = torch.zeros(BIG_N, device="cuda")
    for s, v in vals.items():
        x[s] = float(v)
    return x


ROW_GIB = 18  # one row of 2^32 + 12,345 floats (17.2 GB)


def test_t3_minmax_decimate(torch_cuda):
    """minmax_decimate of the planted zero row, P = 1920 and P = 70,000 (the
    grid caps at 65,535 blocks, so blocks loop over pixels): the pixel of sample
    s is s * P // n in Python integers; an untouched pixel is (0, 0) and a
    planted pixel holds its value on the matching side (bigutil.minmax_expect,
    proved equal to oracle.minmax_decimate in test_large_positions_cpu.py)."""
    torch = torch_cuda
    need(torch, ROW_GIB)
    vals = bu.planted(BIG_N, (1920, 70_000))
    x = planted_row(torch, vals)
    for P in (1920, 70_000):
        vmax, vmin = d.minmax_decimate(x, P)
        emax, emin = bu.minmax_expect(vals, BIG_N, P)
        vmax, vmin = vmax.cpu().numpy(), vmin.cpu().numpy()
        for got, want, side in ((vmax, emax, "max"), (vmin, emin, "min")):
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"P = {P}, {side}: {bad.size} pixels differ, the first {bad[0]}: " \
                                  f"got {got[bad[0]]} want {want[bad[0]]}"
    del x
    release(torch)


@pytest.mark.parametrize("B,O", [(100, 0), (512, 0), (512, bu.P32)])
def test_t3_render_offline_ir_test(torch_cuda, oracle, B, O):
    """render_offline with IR_test and no input rows, L = 2^32 + 12,345: every
    block equals the oracle's block, compared on the device."""
    torch = torch_cuda
    need(torch, ROW_GIB)
    n = d.num_blocks(BIG_N, B) * B
    out = torch.empty((1, n), device="cuda")
    out[0, :4096].view(torch.int32).fill_(S)
    out[0, -4096:].view(torch.int32).fill_(S)
    d.render_offline(None, 1, B, SR, d.Plugin.ir_test(0.9, 0.002), out=out, sample_offset=O, L_file=BIG_N)
    assert blocks_equal(torch, out[0], ramp_tile(torch, oracle, B), step_blocks=(1 << 28) // B)
    del out
    release(torch)


PAIR_GIB = 35  # the planted row and its render (34.4 GB)


def test_t3_render_offline_gain_planted(torch_cuda):
    """render_offline with gain_test on the planted row: the output is zero
    except at the planted indices, where it is float32(v) * float32(0.2)."""
    torch = torch_cuda
    need(torch, PAIR_GIB)
    vals = bu.planted(BIG_N, (1920, 70_000))
    x = planted_row(torch, vals)
    n = d.num_blocks(BIG_N, 512) * 512
    out = torch.empty((1, n), device="cuda")
    d.render_offline(x[None], 1, 512, SR, d.Plugin.gain_test(0.2), out=out)
    nz = torch.zeros((), dtype=torch.int64, device="cuda")
    for i0 in range(0, n, 1 << 30):
        nz += torch.count_nonzero(out[0, i0:i0 + (1 << 30)])
    assert int(nz) == len(vals)
    for s, v in vals.items():
        assert np.float32(out[0, s].item()) == np.float32(v) * np.float32(0.2), s
    del x, out
    release(torch)


def test_t3_stft_largest_hop(torch_cuda):
    """stft_magnitude, N = 8192, H = 2^22 (the call sets no upper limit on the
    hop: check_stft_args asks only H > 0) over the row of 2^32 + 12,345
    samples: 1025 frames, the last starting at sample 2^32.  One impulse in the
    first frame and in each of the last three: those rows follow
    stftutil.check_impulses (its bound), every other row is zero."""
    torch = torch_cuda
    need(torch, ROW_GIB)
    H = 1 << 22
    F = d.stft_frames(BIG_N, N, H)
    assert F == 1025 and (F - 1) * H == bu.P32
    amp = 0.75
    cases = {0: 4095, F - 3: 1000, F - 2: 4097, F - 1: 6001}  # frame: the impulse's sample in it
    x = torch.zeros((1, BIG_N), device="cuda")
    for f, j in cases.items():
        x[0, f * H + j] = amp
    mag = d.stft_magnitude(x, N=N, H=H, window=HANN, K=K)
    assert mag.shape == (1, F, K)
    m = mag[0].cpu().numpy()
    frames = sorted(cases)
    su.check_impulses(m[frames], N, [cases[f] for f in frames], amp, HANN, what="impulses past 2^32")
    rest = np.delete(m, frames, axis=0)
    assert rest.shape[0] == F - 4 and not rest.any()
    del x, mag
    release(torch)


def test_t3_stft8192_rows_past_2_32_floats(torch_cuda, oracle):
    """stft_magnitude, N = 8192, H = 32, F = 1,048,900, ld = 4097 (17.2 GB):
    rows from f = 1,048,321 on start past 2^32 floats, where a row offset
    f * ld formed in 32 bits wraps (a 4 GiB matrix only catches a 32-bit byte
    offset).  The same checks as test_t2_stft8192_rows_past_4gib, around that
    line, for K = 4097 (the computed-window kernel) and K = 4000 (fewer bins than
    N / 2 + 1 take the table-window kernel, which forms its row address itself)."""
    need(torch_cuda, 20)  # the matrix, the 134 MB signal, slice temporaries
    assert bu.first_row_past(4 * bu.P32, 4097) == 1_048_321
    for Kn in (4097, 4000):
        stft_rows_past_4gib(torch_cuda, oracle, 8192, 32, F_ELEMS, (4097,), 0, line_bytes=4 * bu.P32, Kn=Kn)


def test_t3_wav_decode_frames_past_2_32(torch_cuda, oracle):
    """WAV decode at frame indices past 2^32: an int16 mono payload of
    2 * (2^32 + 12,345) bytes, windows of 4099 frames at frame0 = 2^32 - 2000
    and at the end, against the oracle."""
    torch = torch_cuda
    need(torch, 10)  # the 8.6 GB payload
    payload = random_bytes(torch, 2 * BIG_N)
    check_wav_windows(torch, oracle, payload, 16, 1, False, (bu.P32 - 2000, bu.P32 - 2001, BIG_N - 4099))
    del payload
    release(torch)
