"""The cached spectrum row of the fused IR_test STFT (DSP_RESULT_SPECTRUM_CACHE).

When H % B == 0 every frame of a call has the same 4097 magnitudes.  Outside
stream capture the library keeps that row per device, keyed by what it depends
on, and a call's launch (stft8192_rows_kernel) only stores: the hops, then the
row once per frame as aligned 16-byte pieces.  A miss computes the row with the
one-frame-per-wave kernel, so every comparison here is bit for bit against the
same call with DSP_EXEC_EVERY_FRAME, which runs that kernel on every frame.

Small calls do not take the path by themselves: DSP_DEBUG_SPECTRUM_CACHE = 1
forces it wherever it is valid (2 turns it off), DSP_DEBUG_ROW_RUN sets the
frames per wave of the store-only launch.

dsp_exec.sample_offset must be a multiple of B (the call refuses anything
else, checked below), so the sample phase goff mod B of the row's key is always
0 today; the offsets used here are multiples of B.
"""
import contextlib
import ctypes as C
import gc
import itertools
import os
import struct

import numpy as np
import pytest

import dspbench as d
import dspbench._lib as L
import rowsutil as ru
from dspbench.api import last_result

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
IR_CO = os.path.join(os.path.dirname(HERE), "dsp-bench_amd", "modules", "mod_IR_test.co")
N = 8192
K = 4097
SR = 48000.0
# include/dspbench/dspbench.h
DSP_RESULT_SPECTRUM_CACHE = 0x10
DSP_DEBUG_SPECTRUM_CACHE = 4
DSP_DEBUG_ROW_RUN = 5
REUSE = L.DSP_RESULT_FRAME_REUSE
BOTH = REUSE | DSP_RESULT_SPECTRUM_CACHE


def _set(what, value):
    L.check(L.lib().dsp_debug_set(what, value), "dsp_debug_set")


@contextlib.contextmanager
def hooks(cache=1, row_run=0, frame_run=0):
    _set(DSP_DEBUG_SPECTRUM_CACHE, cache)
    _set(DSP_DEBUG_ROW_RUN, row_run)
    _set(L.DSP_DEBUG_FRAME_RUN, frame_run)
    try:
        yield
    finally:
        _set(DSP_DEBUG_SPECTRUM_CACHE, 0)
        _set(DSP_DEBUG_ROW_RUN, 0)
        _set(L.DSP_DEBUG_FRAME_RUN, 0)


def load_module():
    with open(IR_CO, "rb") as f:
        mod = d.module.Module(f.read())
    mod.initialize_state(mod.default_parameters(), 3, SR)
    return mod


@pytest.fixture(scope="module")
def source():
    """IR_test.cpp compiled unchanged (build() compiles it from the reference's
    sources where they are present; without it the cases that need it say so)."""
    if not os.path.exists(IR_CO):
        pytest.skip("dsp-bench_amd/modules/mod_IR_test.co is not built")
    return load_module()


def enum_pair(gain=0.9, step=0.002):
    return d.Plugin.ir_test(gain, step), d.Plugin.ir_test(gain, step, every_frame=True)


def source_pair(mod, params=None):
    params = mod.default_parameters() if params is None else params
    return mod.plugin(params, "IR_test"), mod.plugin(params, "IR_test", every_frame=True)


def buffers(torch, Cn, B, F, H=4096, ld=K, phase=0, tail=False):
    """(L_file, file, out rows, mag rows): NaN-sentinel rows with guards
    (rowsutil), the first magnitude row `phase` floats past a 16-byte boundary,
    `tail`: 17 samples past the last frame, in a block no frame owns."""
    L_ = (F - 1) * H + N + (17 if tail else 0)
    Lr = (L_ + B - 1) // B * B
    assert d.stft_frames(Lr, N, H) == F
    out = ru.Rows(Cn, Lr, off=0, torch=torch)
    mag = ru.Rows(Cn, F * ld, off=phase, torch=torch)
    file = torch.zeros((Cn, L_ + (L_ & 1)), device="cuda")
    return L_, file, out, mag


def call(torch, plugin, Cn, B, F, H=4096, ld=K, phase=0, tail=False, sample_offset=0, window=d.DSP_WIN_HANN):
    L_, file, out, mag = buffers(torch, Cn, B, F, H, ld, phase, tail)
    d.render_stft(file, Cn, B, SR, plugin, H=H, window=window, ld=ld, out=out.view, mag=mag.frames(F, ld),
                  sample_offset=sample_offset, L_file=L_)
    res = last_result()
    torch.cuda.synchronize()
    return out, mag, res, (F, ld)


def check_rows(got, shape):
    """Every float of the render and of every row's K bins written, nothing else touched."""
    out, mag, _, (F, ld) = got
    out.check_output()
    mag.check_output(F * ld, K, ld)


def same(a, b):
    return ru.same_bits(a[0].numpy(), b[0].numpy()) and ru.same_bits(a[1].numpy(), b[1].numpy())


def assert_cached_same(torch, pair, *args, bits=BOTH, **kw):
    cached, every = pair
    got = call(torch, cached, *args, **kw)
    want = call(torch, every, *args, **kw)
    what = (args, kw)
    assert got[2] & BOTH == bits, (hex(got[2]), what)
    assert want[2] & BOTH == 0, (hex(want[2]), what)
    check_rows(got, what)
    assert same(got, want), what
    return got


@pytest.mark.parametrize("row_run", [1, 2, 4])
@pytest.mark.parametrize("B", [128, 512])
def test_shapes(torch_cuda, B, row_run):
    """C, F, tail, ld (every row phase and phase step), sample_offset, at run
    lengths 1, 2 and 4: the every-frame call's bits, guard rows and the gaps
    between rows intact."""
    torch = torch_cuda
    cases = list(itertools.product((1, 2), (1, 2, 5, 9), (False, True)))
    with hooks(cache=1, row_run=row_run):
        pair = enum_pair()
        for i, (Cn, F, tail) in enumerate(cases):
            for j, ld in enumerate((4097, 4098, 4100, 4104)):
                off = (0, 3 * B, 7 * B, B)[(i + j) % 4]
                assert_cached_same(torch, pair, Cn, B, F, ld=ld, phase=(i + j) % 4, tail=tail, sample_offset=off)


def other_hops_and_periods(torch, pair):
    with hooks(cache=1):
        for Cn, B, H, tail in ((3, 256, 2048, True), (2, 1024, 4096, False), (1, 2048, 4096, True),
                               (2, 2, 4096, False), (2, 512, 1024, True)):
            assert_cached_same(torch, pair, Cn, B, 5, H=H, ld=4099, phase=1, tail=tail, sample_offset=5 * B)


def test_other_hops_and_periods(torch_cuda):
    """The other PER instantiations (B = 2, 256, 1024, 2048), hops of a half
    and a quarter frame (the general render branch), three channels."""
    other_hops_and_periods(torch_cuda, enum_pair())


def test_other_hops_and_periods_source(torch_cuda, source):
    """The same with IR_test.cpp compiled unchanged."""
    other_hops_and_periods(torch_cuda, source_pair(source))


def test_offset_must_be_a_multiple_of_B(torch_cuda):
    """The sample phase of the key: offsets that are no multiple of B are
    refused before any launch, with and without the cached path."""
    for mode in (1, 2):
        with hooks(cache=mode):
            for off in (2, 510, 512 * 3 + 6):
                with pytest.raises(Exception, match="multiple of B"):
                    call(torch_cuda, enum_pair()[0], 1, 512, 2, sample_offset=off)


def alternate(torch, variants):
    """Two rounds over the variants, call by call; {name: magnitudes [C, F, K]}."""
    mags = {}
    with hooks(cache=1):
        for rnd in range(2):
            for name, v in variants.items():
                v = dict(v)
                pair, B = v.pop("pair"), v.pop("B", 512)
                got = assert_cached_same(torch, pair, 2, B, 3, ld=4098, phase=rnd, **v)
                mags[name] = got[1].numpy(3 * 4098).reshape(2, 3, 4098)[:, :, :K]
    return mags


def test_key_alternating(torch_cuda):
    """Calls that differ in one part of the key, alternated call by call on
    one device: each equals its own every-frame result (so none got another's
    row), and the rows of different keys do differ."""
    mags = alternate(torch_cuda, {
        "base": dict(pair=enum_pair(0.9, 0.002)),
        "params": dict(pair=enum_pair(0.7, 0.003)),
        "thirds": dict(pair=enum_pair(1.0 / 3.0, 1e-5 / 3.0)),
        "hamming": dict(pair=enum_pair(0.9, 0.002), window=d.DSP_WIN_HAMMING),
        "offset": dict(pair=enum_pair(0.9, 0.002), window=d.DSP_WIN_HANN, sample_offset=512 * 3),
        "B256": dict(pair=enum_pair(0.9, 0.002), B=256),
    })
    for other in ("params", "thirds", "hamming", "B256"):
        assert not np.array_equal(mags["base"], mags[other]), other
    assert np.array_equal(mags["base"], mags["offset"])  # a whole number of blocks later: the same phase


def test_key_alternating_source(torch_cuda, source):
    """The compiled source with two parameter sets (IR_test.cpp:
    Parameters{gain, step}) alternated with the enum plugin."""
    mags = alternate(torch_cuda, {
        "enum": dict(pair=enum_pair(0.9, 0.002)),
        "source": dict(pair=source_pair(source, struct.pack("<ff", 0.9, 0.002))),
        "source_params": dict(pair=source_pair(source, struct.pack("<ff", 0.7, 0.003))),
    })
    assert np.array_equal(mags["enum"], mags["source"])  # the source's block is the enum's
    assert not np.array_equal(mags["source"], mags["source_params"])


def test_rebuilt_module_tables(torch_cuda, source):
    """A module loaded again, and a module whose table cache evicted the block
    (5 parameter sets against 4 entries): the first parameters again, and every
    call on the way, is right."""
    torch = torch_cuda
    with hooks(cache=1):
        first = source_pair(source)
        assert_cached_same(torch, first, 1, 512, 2)
        again = load_module()
        assert_cached_same(torch, source_pair(again), 1, 512, 2)
        for i in range(5):
            assert_cached_same(torch, source_pair(source, struct.pack("<ff", 0.8 - 0.01 * i, 0.001)), 1, 512, 2)
        assert_cached_same(torch, first, 1, 512, 2)
        del again
        gc.collect()


def test_row_eviction(torch_cuda):
    """More keys than the device keeps rows (9 against 8), then the first
    again: its row was retired and is computed again."""
    with hooks(cache=1):
        for i in range(9):
            assert_cached_same(torch_cuda, enum_pair(0.6 - 0.01 * i, 0.0015), 1, 512, 2)
        assert_cached_same(torch_cuda, enum_pair(0.6, 0.0015), 1, 512, 2)


def test_two_streams(torch_cuda):
    """The miss on one stream and the hit on another, issued back to back
    with no synchronisation by the caller: the hit waits for the row.  The
    miss's stream is busy with other work first, so the row does not exist yet
    when the hit is enqueued; a hit that did not wait would store whatever the
    fresh row held."""
    torch = torch_cuda
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    shapes = (dict(Cn=2, B=512, F=9), dict(Cn=2, B=512, F=9, ld=4098, phase=3))
    with hooks(cache=1):
        cached, every = enum_pair(0.4321, 0.00123)  # a key no other test uses
        want = [call(torch, every, **kw) for kw in shapes]
        bufs = [buffers(torch, **kw) for kw in shapes]
        warm = [buffers(torch, 1, 512, 2) for _ in range(2)]
        torch.cuda.synchronize()
        for s, (L_, file, out, mag) in zip((s1, s2), warm):  # the streams' scratch, with another key
            d.render_stft(file, 1, 512, SR, enum_pair()[0], ld=K, out=out.view, mag=mag.frames(2, K), L_file=L_,
                          stream=s.cuda_stream)
        ballast = torch.zeros(1 << 28, device="cuda")  # 1 GiB: a pass over it takes a fraction of a millisecond
        torch.cuda.synchronize()  # everything above; nothing below until both calls are enqueued
        with torch.cuda.stream(s1):
            for _ in range(100):
                ballast.add_(1.0)
        res = []
        for s, kw, (L_, file, out, mag) in zip((s1, s2), shapes, bufs):
            F, ld = kw["F"], kw.get("ld", K)
            d.render_stft(file, kw["Cn"], kw["B"], SR, cached, ld=ld, out=out.view, mag=mag.frames(F, ld), L_file=L_,
                          stream=s.cuda_stream)
            res.append(last_result())
        busy = not s1.query()  # s1 had not finished (so the row was not there) when the hit was enqueued
        torch.cuda.synchronize()
        assert busy, "the miss's stream was idle before the hit was enqueued: the test did not test the wait"
        for r, kw, (L_, file, out, mag), w in zip(res, shapes, bufs, want):
            assert r & BOTH == BOTH, (hex(r), kw)
            got = (out, mag, r, (kw["F"], kw.get("ld", K)))
            check_rows(got, kw)
            assert same(got, w), kw


def test_capture(torch_cuda):
    """A call under capture takes the reuse launch (no cached bit, nothing
    allocated or waited for), gives the eager call's bits, and so does the replay."""
    torch = torch_cuda
    with hooks(cache=1, frame_run=4):
        cached, every = enum_pair()
        L_, file, out, mag = buffers(torch, 2, 512, 9)
        want = call(torch, every, 2, 512, 9)

        def run():
            d.render_stft(file, 2, 512, SR, cached, ld=K, out=out.view, mag=mag.frames(9, K), L_file=L_)
            return last_result()

        assert run() & BOTH == BOTH  # eager: the cached row
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm the capture stream's scratch
            run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            res = run()
        assert res & BOTH == REUSE, hex(res)
        for _ in range(2):
            out.whole.view(torch.int32).fill_(int(ru.SENTINEL))
            mag.whole.view(torch.int32).fill_(int(ru.SENTINEL))
            g.replay()
            torch.cuda.synchronize()
            check_rows((out, mag, res, (9, K)), "replay")
            assert same((out, mag), want)
        del g
        gc.collect()


def test_fallbacks(torch_cuda):
    """H % B != 0, B off the periodic path, DSP_EXEC_EVERY_FRAME (every
    reference call here), the path turned off and a forced frame run without
    the force switch: the old launches, the cached bit clear, the same outputs."""
    torch = torch_cuda
    with hooks(cache=1):
        assert_cached_same(torch, enum_pair(), 2, 512, 5, H=3968, bits=0)  # 3968 % 512 != 0
        assert_cached_same(torch, enum_pair(), 2, 4096, 5, bits=0)         # B > 2048: no periodic frame
    with hooks(cache=2):
        assert_cached_same(torch, enum_pair(), 2, 512, 5, bits=0)
    with hooks(cache=2, frame_run=4):
        assert_cached_same(torch, enum_pair(), 2, 512, 5, bits=REUSE)
    with hooks(cache=0, frame_run=4):  # the hook asks for the reuse launch
        assert_cached_same(torch, enum_pair(), 2, 512, 5, bits=REUSE)
    with hooks(cache=0):  # a call too short for frame reuse: one frame per wave
        assert_cached_same(torch, enum_pair(), 2, 512, 5, bits=0)


def test_verify_class_falls_back(torch_cuda, source):
    """DSP_EXEC_VERIFY_CLASS (a GENERIC plugin): the old launch, verified."""
    with hooks(cache=1):
        verify = source.plugin(source.default_parameters(), "IR_test", verify=True)
        got = assert_cached_same(torch_cuda, (verify, source_pair(source)[1]), 2, 512, 5, bits=0)
        assert got[2] & L.DSP_RESULT_VERIFIED


def test_one_timed_launch(torch_cuda):
    """A miss and a hit each record one timed launch (the miss's one-frame
    launch is outside the timed region) of C F (4 H + 4 K) bytes plus the tail."""
    torch = torch_cuda
    lib = L.lib()
    Cn, B, F, H = 2, 512, 9, 4096
    with hooks(cache=1):
        pair = enum_pair(0.2468, 0.00135)  # a fresh key: the first call misses
        for _ in range(2):
            lib.dsp_kernel_timing(None, None, None)
            lib.dsp_kernel_timing_enable(1)
            try:
                got = call(torch, pair[0], Cn, B, F, tail=True)
            finally:
                lib.dsp_kernel_timing_enable(0)
            ms, n, nbytes = C.c_double(), C.c_uint64(), C.c_uint64()
            L.check(lib.dsp_kernel_timing(C.byref(ms), C.byref(n), C.byref(nbytes)), "dsp_kernel_timing")
            assert got[2] & BOTH == BOTH
            assert n.value == 1
            Lr = got[0].n
            assert nbytes.value == Cn * F * (4 * H + 4 * K) + Cn * (Lr - F * H) * 4
