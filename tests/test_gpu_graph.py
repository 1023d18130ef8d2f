"""Stream capture: the library's calls are stream-ordered launches with no
host synchronisation once a device's constant tables exist, so a caller can
capture them into a HIP graph (here through torch.cuda.graph, which captures
the current stream) and replay the whole render + STFT of a file with one
launch -- what an application rendering many short files repeatedly wants.
Replays must give the eager call's bits, and follow new input contents.
"""
import gc

import numpy as np
import pytest

import dspbench as d

pytestmark = pytest.mark.gpu


def _refused_capture(torch, fn):
    """Capture fn() on a fresh stream, expecting the library to refuse it;
    returns the error text.  The failed graph is destroyed and collected here,
    outside any capture (a graph object collected during a later capture
    would free its pool mid-capture)."""
    gc.collect()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    msg = None
    try:
        with torch.cuda.graph(g, stream=side):
            fn()
    except Exception as e:  # noqa: BLE001
        msg = str(e)
    torch.cuda.synchronize()
    del g
    gc.collect()
    assert msg is not None, "the capture was not refused"
    return msg


def _eager_and_graph(torch, fn, x):
    """fn(x) -> tensors: eager results, then a captured graph's replay on
    the same input and on a changed one (compared with eager on that)."""
    want = [t.clone() for t in fn(x)]          # eager; also creates the device tables
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):              # warm the capture stream's scratch
        fn(x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):     # capture on the warmed stream
        outs = fn(x)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, want):
        assert torch.equal(a, b)
    x.mul_(-0.5)                               # new contents, same buffer
    want2 = [t.clone() for t in fn(x)]
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, want2):
        assert torch.equal(a, b)
    return outs


@pytest.mark.parametrize("plugin", ["gain_test", "IR_test", "no_op"])
@pytest.mark.parametrize("B", [512, 384])
def test_render_stft_captured(torch_cuda, plugin, B):
    torch = torch_cuda
    mk = {"gain_test": lambda: d.Plugin.gain_test(0.7), "IR_test": lambda: d.Plugin.ir_test(0.9, 0.002),
          "no_op": lambda: d.Plugin.no_op()}[plugin]
    L = 8192 * 7 + 300
    x = torch.from_numpy(np.random.default_rng(B).uniform(-1, 1, (2, L)).astype(np.float32)).cuda()
    nb = d.num_blocks(L, B)
    out = torch.empty((2, nb * B), device="cuda")
    mag = torch.empty((2, d.stft_frames(nb * B, 8192, 4096), 4097), device="cuda")
    p = mk()

    def fn(xx):
        return d.render_stft(xx, 2, B, 48000.0, p, out=out, mag=mag)
    _eager_and_graph(torch, fn, x)


def test_stft_and_render_chain_captured(torch_cuda):
    """Two calls in one graph: a render, then the STFT of another signal."""
    torch = torch_cuda
    L = 8192 * 5
    x = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (2, L)).astype(np.float32)).cuda()
    out = torch.empty((2, L), device="cuda")
    mag = torch.empty((2, d.stft_frames(L, 8192, 4096), 4097), device="cuda")
    p = d.Plugin.gain_test(0.25)

    def fn(xx):
        r = d.render_offline(xx, 2, 512, 48000.0, p, out=out)
        m = d.stft_magnitude(xx, out=mag)
        return r, m
    _eager_and_graph(torch, fn, x)


def test_capture_on_a_cold_stream_is_refused_cleanly(torch_cuda):
    """A shape that needs per-stream scratch, captured on a stream that never
    ran it eagerly: a clear DSP_ERR_INVALID, not an allocation inside the
    capture (IR_test with a step whose ramp is not closed-form, B = 384)."""
    torch = torch_cuda
    L = 8192 * 3
    x = torch.zeros((2, L), device="cuda")
    p = d.Plugin.ir_test(0.8, 0.0013)
    d.render_stft(x, 2, 384, 48000.0, p)      # device tables exist
    torch.cuda.synchronize()
    msg = _refused_capture(torch, lambda: d.render_stft(x, 2, 384, 48000.0, p))
    assert "eager call" in msg or "capture" in msg


# a one-gain plugin of this test's own (block class GAIN): the test needs no
# module built from sources outside the repository
PLAIN_GAIN_SRC = r'''
#include "plugin_header.h"
struct Parameters { FLOAT_PARAM(0.0f, 2.0f) level; };
struct State {};
Parameters default_parameters() { Parameters p = {0.3f}; return p; }
State initialize_state(const Parameters &p, const unsigned C, const float sr, void *ctx) { State s; return s; }
void audio_callback(const Parameters &p, State &st, float **out, const u32 C, const u32 B, const real32 sr) {
    for (u32 c = 0; c < C; ++c)
        for (u32 s = 0; s < B; ++s) out[c][s] *= p.level;
}
'''


def test_generic_plugin_capture_is_refused(torch_cuda):
    """A GENERIC plugin run by its callback has its Parameters go up through a
    host-staged copy, which a graph replay would not repeat: capturing its
    render is refused with a clear error, and the eager call still works
    afterwards.  The same plugin run as its block class (here PLAIN_GAIN_SRC,
    compiled by the test: the gain map, known from an eager call) captures and
    replays bit for bit."""
    torch = torch_cuda
    mod = d.module.Module(d.module.compile_source(PLAIN_GAIN_SRC, "plain_gain.cpp"))
    params = mod.default_parameters()
    mod.initialize_state(params, 2, 48000.0)
    p = mod.plugin(params, "plain_gain", specialize=False)
    x = torch.rand((2, 4096), device="cuda")
    want = d.render_offline(x, 2, 512, 48000.0, p).clone()
    torch.cuda.synchronize()
    msg = _refused_capture(torch, lambda: d.render_offline(x, 2, 512, 48000.0, p))
    assert "captured" in msg, msg
    assert torch.equal(d.render_offline(x, 2, 512, 48000.0, p), want)
    ps = mod.plugin(params, "plain_gain")
    out = torch.empty((2, 4096), device="cuda")

    def fn(xx):
        return (d.render_offline(xx, 2, 512, 48000.0, ps, out=out),)
    _eager_and_graph(torch, fn, x)
    assert mod.block_class(params, 2, 512, 48000.0)[0] == "gain", mod.facts


def test_first_use_table_under_capture_is_refused(torch_cuda):
    """A window table first needed inside a capture (a kind / N no eager call
    used) is refused with the 'eager call first' error instead of uploading
    on the legacy stream mid-capture; after one eager call the capture works."""
    torch = torch_cuda
    x = torch.rand((1, 3 * 2048), device="cuda")  # (N = 8: a window no other test creates)
    msg = _refused_capture(torch, lambda: d.stft_magnitude(x, N=8, H=3, window=d.DSP_WIN_RECT, K=5))
    assert "eager call" in msg, msg
    side = torch.cuda.Stream()
    want = d.stft_magnitude(x, N=8, H=3, window=d.DSP_WIN_RECT, K=5).clone()
    out = torch.empty_like(want)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d.stft_magnitude(x, N=8, H=3, window=d.DSP_WIN_RECT, K=5, out=out)
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=side):
        d.stft_magnitude(x, N=8, H=3, window=d.DSP_WIN_RECT, K=5, out=out)
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
