"""The store-only launch of a cached spectrum row (stft8192_rows_kernel): its
pacing and the events of its hit path.

The launch's pacing (DSP_DEBUG_ROW_PACE: a sleep between a wave's hop stores
and its row stores, an LDS pad that sets how many waves a compute unit holds)
changes when stores are issued, never what is stored; a hit enqueues no wait
once the row's ready event has been seen completed, and the row's lifetime
event completes with the launch itself.  Every comparison is bit for bit with
the same call under DSP_EXEC_EVERY_FRAME (one FFT per frame, no cache), on
NaN-filled rows with guards (rowsutil), so a word written outside a row or
left unwritten is caught.  DSP_DEBUG_SPECTRUM_CACHE = 1 forces the row path at
any length.
"""
import contextlib
import gc
import itertools

import pytest

import dspbench as d
import dspbench._lib as L
import rowsutil as ru
from dspbench.api import last_result

pytestmark = pytest.mark.gpu

N = 8192
K = 4097
SR = 48000.0
# include/dspbench/dspbench.h
DSP_RESULT_SPECTRUM_CACHE = 0x10
DSP_DEBUG_SPECTRUM_CACHE = 4
DSP_DEBUG_ROW_PACE = 6
PACE_RECORD = 1 << 16
REUSE = L.DSP_RESULT_FRAME_REUSE
BOTH = REUSE | DSP_RESULT_SPECTRUM_CACHE
# every value the build accepts: nap 0..16, waves 3..9, with and without the recorded lifetime event
PACES = [nap | waves << 8 | rec for rec in (0, PACE_RECORD) for waves in range(3, 10) for nap in range(17)]


def _set(what, value):
    L.check(L.lib().dsp_debug_set(what, value), "dsp_debug_set")


@contextlib.contextmanager
def hooks(cache=1, pace=0, frame_run=0):
    _set(DSP_DEBUG_SPECTRUM_CACHE, cache)
    _set(DSP_DEBUG_ROW_PACE, pace)
    _set(L.DSP_DEBUG_FRAME_RUN, frame_run)
    try:
        yield
    finally:
        _set(DSP_DEBUG_SPECTRUM_CACHE, 0)
        _set(DSP_DEBUG_ROW_PACE, 0)
        _set(L.DSP_DEBUG_FRAME_RUN, 0)


def enum_pair(gain=0.9, step=0.002):
    return d.Plugin.ir_test(gain, step), d.Plugin.ir_test(gain, step, every_frame=True)


def buffers(torch, Cn, B, F, H=4096, ld=K, phase=0, tail=False):
    """(L_file, file, out rows, mag rows): NaN-sentinel rows with guards, the
    first magnitude row `phase` floats past a 16-byte boundary, `tail`: 17
    samples past the last frame, in a block no frame owns."""
    L_ = (F - 1) * H + N + (17 if tail else 0)
    Lr = (L_ + B - 1) // B * B
    assert d.stft_frames(Lr, N, H) == F
    out = ru.Rows(Cn, Lr, off=0, torch=torch)
    mag = ru.Rows(Cn, F * ld, off=phase, torch=torch)
    file = torch.zeros((Cn, L_ + (L_ & 1)), device="cuda")
    return L_, file, out, mag


def enqueue(plugin, buf, Cn, B, F, H=4096, ld=K, sample_offset=0, stream=None, **_):
    L_, file, out, mag = buf
    kw = {} if stream is None else {"stream": stream.cuda_stream}
    d.render_stft(file, Cn, B, SR, plugin, H=H, window=d.DSP_WIN_HANN, ld=ld, out=out.view, mag=mag.frames(F, ld),
                  sample_offset=sample_offset, L_file=L_, **kw)
    return last_result()


def call(torch, plugin, Cn, B, F, **kw):
    buf = buffers(torch, Cn, B, F, kw.get("H", 4096), kw.get("ld", K), kw.get("phase", 0), kw.get("tail", False))
    res = enqueue(plugin, buf, Cn, B, F, **kw)
    torch.cuda.synchronize()
    return buf[2], buf[3], res


def check_rows(out, mag, F, ld):
    """Every float of the render and of every row's K bins written, nothing else touched."""
    out.check_output()
    mag.check_output(F * ld, K, ld)


def same_words(torch, a, b):
    """Two Rows allocations hold the same bits, guards and gaps included (compared on the device)."""
    return torch.equal(a.whole.view(torch.int32), b.whole.view(torch.int32))


def assert_cached_same(torch, pair, Cn, B, F, **kw):
    cached, every = pair
    out, mag, res = call(torch, cached, Cn, B, F, **kw)
    wout, wmag, wres = call(torch, every, Cn, B, F, **kw)
    what = (Cn, B, F, kw)
    assert res & BOTH == BOTH, (hex(res), what)
    assert wres & BOTH == 0, (hex(wres), what)
    check_rows(out, mag, F, kw.get("ld", K))
    assert same_words(torch, out, wout) and same_words(torch, mag, wmag), what


@pytest.mark.parametrize("Cn", [1, 2, 3])
@pytest.mark.parametrize("H", [4096, 2048])
def test_shapes(torch_cuda, H, Cn):
    """F = 1, 2, 5, 70, 257 (the last two: more waves than one XCD's share of a
    compute unit's slots at C = 1), every ld in 4097..4100 (every dword phase
    and phase step of a row) with and without a render tail, sample_offset 0
    and 3 B, at B = 512: the every-frame call's bits, guards and gaps intact."""
    torch = torch_cuda
    B = 512
    with hooks(cache=1):
        pair = enum_pair()
        for i, (F, tail) in enumerate(itertools.product((1, 2, 5, 70, 257), (False, True))):
            for j, ld in enumerate((4097, 4098, 4099, 4100)):
                for k, off in enumerate((0, 3 * B)):
                    assert_cached_same(torch, pair, Cn, B, F, H=H, ld=ld, phase=(i + j + k) % 4, tail=tail,
                                       sample_offset=off)


def test_every_pace_same_bytes(torch_cuda):
    """Every DSP_DEBUG_ROW_PACE value the build accepts writes what the default
    writes -- which is what the every-frame call writes -- at a shape with more
    waves than a compute unit holds, an odd ld, a tail and an offset."""
    torch = torch_cuda
    shape = dict(Cn=2, B=512, F=70, ld=4099, phase=1, tail=True, sample_offset=3 * 512)
    pair = enum_pair()
    with hooks(cache=1):
        wout, wmag, wres = call(torch, pair[1], **shape)
        dout, dmag, dres = call(torch, pair[0], **shape)
    assert wres & BOTH == 0 and dres & BOTH == BOTH
    check_rows(dout, dmag, 70, 4099)
    assert same_words(torch, dout, wout) and same_words(torch, dmag, wmag)
    for pace in PACES:
        with hooks(cache=1, pace=pace):
            out, mag, res = call(torch, pair[0], **shape)
        assert res & BOTH == BOTH, hex(pace)
        assert same_words(torch, out, dout) and same_words(torch, mag, dmag), hex(pace)


def test_pace_values_refused():
    """Outside nap 0..16 | waves 3..9 << 8 [| 1 << 16] the hook refuses and keeps its value."""
    lib = L.lib()
    try:
        _set(DSP_DEBUG_ROW_PACE, 0x408)
        for bad in (0x208, 0xA00, 0x911, 0x8, 1 << 17 | 0x900, 1 << 32 | 0x900):
            assert lib.dsp_debug_set(DSP_DEBUG_ROW_PACE, bad) != 0, hex(bad)
        import ctypes as C
        v = C.c_uint64()
        L.check(lib.dsp_debug_get(DSP_DEBUG_ROW_PACE, C.byref(v)), "dsp_debug_get")
        assert v.value == 0x408
    finally:
        _set(DSP_DEBUG_ROW_PACE, 0)


def busy_streams(torch, streams):
    """Some milliseconds of other work on each stream, so that what is enqueued next stays queued."""
    ballast = torch.zeros(1 << 28, device="cuda")  # 1 GiB: a pass over it takes a fraction of a millisecond
    torch.cuda.synchronize()
    for s in streams:
        with torch.cuda.stream(s):
            for _ in range(60):
                ballast.add_(1.0)
    return ballast


def test_two_streams_first_hit_and_later_hits(torch_cuda):
    """The miss on one stream, and at once the hit on another: the row's ready
    event is pending, so this hit must wait for it (no sticky flag yet).  After
    the device has finished, hits on both streams see the event completed and
    enqueue no wait.  All of them give the every-frame call's bits."""
    torch = torch_cuda
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    shapes = (dict(Cn=2, B=512, F=9), dict(Cn=2, B=512, F=9, ld=4098, phase=3))
    with hooks(cache=1):
        cached, every = enum_pair(0.4567, 0.00117)  # a key no other test uses
        want = [call(torch, every, **kw) for kw in shapes]
        for s in (s1, s2):  # the streams' scratch, with another key
            enqueue(enum_pair()[0], buffers(torch, 1, 512, 2), 1, 512, 2, stream=s)
        bufs = [buffers(torch, **kw) for kw in shapes]
        keep = busy_streams(torch, (s1,))
        res = [enqueue(cached, buf, stream=s, **kw) for s, kw, buf in zip((s1, s2), shapes, bufs)]
        busy = not s1.query()  # the miss had not run (the row was not there) when the hit was enqueued
        torch.cuda.synchronize()
        assert busy, "the miss's stream was idle before the hit was enqueued: the test did not test the wait"
        later = []
        for rnd in range(2):  # the first of these sets the flag, the rest rely on it
            for s, kw in zip((s2, s1), shapes):
                buf = buffers(torch, **kw)
                later.append((enqueue(cached, buf, stream=s, **kw), kw, buf, want[shapes.index(kw)]))
        torch.cuda.synchronize()
        del keep
    for r, kw, buf, w in [(r, kw, buf, w) for r, kw, buf, w in zip(res, shapes, bufs, want)] + later:
        assert r & BOTH == BOTH, (hex(r), kw)
        check_rows(buf[2], buf[3], kw["F"], kw.get("ld", K))
        assert same_words(torch, buf[2], w[0]) and same_words(torch, buf[3], w[1]), kw


def test_nine_keys_while_launches_are_queued(torch_cuda):
    """Nine distinct keys in turn on two busy streams -- one more than the
    device keeps rows, so the first is retired while the launch that reads it is
    still queued -- then the first key again (a miss that must not take the
    retired row while its reader is in flight).  Every call's output is its own
    every-frame result."""
    torch = torch_cuda
    s = (torch.cuda.Stream(), torch.cuda.Stream())
    shape = dict(Cn=1, B=512, F=3, ld=4099, phase=2, tail=True)
    pairs = [enum_pair(0.61 - 0.01 * i, 0.0017) for i in range(9)]
    pairs.append(pairs[0])
    with hooks(cache=1):
        want = [call(torch, every, **shape) for _, every in pairs[:9]]
        want.append(want[0])
        for st in s:  # the streams' scratch, with another key
            enqueue(enum_pair()[0], buffers(torch, 1, 512, 2), 1, 512, 2, stream=st)
        bufs = [buffers(torch, **shape) for _ in pairs]
        keep = busy_streams(torch, s)
        res = [enqueue(cached, buf, stream=s[i % 2], **shape) for i, ((cached, _), buf) in enumerate(zip(pairs, bufs))]
        busy = not s[0].query() and not s[1].query()
        torch.cuda.synchronize()
        del keep
        assert busy, "the streams were idle before the last call was enqueued: no launch was in flight at the eviction"
        # and once more with everything completed: retired rows are recycled
        for (cached, every) in pairs[:3]:
            assert_cached_same(torch, (cached, every), **shape)
    for r, buf, w in zip(res, bufs, want):
        assert r & BOTH == BOTH, hex(r)
        check_rows(buf[2], buf[3], shape["F"], shape["ld"])
        assert same_words(torch, buf[2], w[0]) and same_words(torch, buf[3], w[1])


def test_hit_under_capture_takes_the_reuse_launch(torch_cuda):
    """A key whose row is cached and seen ready: the call under stream capture
    still takes the reuse launch (no cached bit, no event, no wait), and the
    replay gives the every-frame bits."""
    torch = torch_cuda
    with hooks(cache=1, frame_run=4):
        cached, every = enum_pair()
        buf = buffers(torch, 2, 512, 9)
        want = call(torch, every, 2, 512, 9)
        for _ in range(2):  # a miss or a hit, then a hit with the flag set
            assert enqueue(cached, buf, 2, 512, 9) & BOTH == BOTH
            torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm the capture stream's scratch
            enqueue(cached, buf, 2, 512, 9)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            res = enqueue(cached, buf, 2, 512, 9)
        assert res & BOTH == REUSE, hex(res)
        buf[2].whole.view(torch.int32).fill_(int(ru.SENTINEL))
        buf[3].whole.view(torch.int32).fill_(int(ru.SENTINEL))
        g.replay()
        torch.cuda.synchronize()
        check_rows(buf[2], buf[3], 9, K)
        assert same_words(torch, buf[2], want[0]) and same_words(torch, buf[3], want[1])
        del g
        gc.collect()
