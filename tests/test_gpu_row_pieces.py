"""Row stores of a reused run as aligned 16-byte pieces (stft_pk PER path).

A wave that owns a run of G frames stages each 4097-bin row in its LDS tile at
the row's dword phase and stores it as aligned 16-byte pieces plus at most 3
head and 3 tail dwords; the run's render hops go out before the FFT.  The
values and addresses are those of the one-frame-per-wave kernel
(DSP_EXEC_EVERY_FRAME, untouched), so every comparison here is bit for bit
against the same call with every_frame=True.  Small calls get G = 1 from the
library, so G is set through the DSP_DEBUG_FRAME_RUN hook.
"""
import os

import pytest

import dspbench as d
import dspbench._lib as L
from dspbench.api import last_result

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
IR_CO = os.path.join(os.path.dirname(HERE), "dsp-bench_amd", "modules", "mod_IR_test.co")
N = 8192
K = 4097
G = 4  # frames per wave (the hook): the library's own run length
SR = 48000.0
OUT_GUARD = 4098


@pytest.fixture
def frame_run():
    L.check(L.lib().dsp_debug_set(L.DSP_DEBUG_FRAME_RUN, G), "dsp_debug_set")
    yield
    L.check(L.lib().dsp_debug_set(L.DSP_DEBUG_FRAME_RUN, 0), "dsp_debug_set")


@pytest.fixture(scope="module")
def plugins():
    """(name, plugin with reuse, plugin with every frame): the enum kind and,
    where it is built, IR_test.cpp compiled unchanged."""
    out = [("enum", d.Plugin.ir_test(), d.Plugin.ir_test(every_frame=True))]
    if os.path.exists(IR_CO):
        with open(IR_CO, "rb") as f:
            mod = d.module.Module(f.read())
        params = mod.default_parameters()
        mod.initialize_state(params, 3, SR)
        out.append(("source", mod.plugin(params, "IR_test"), mod.plugin(params, "IR_test", every_frame=True)))
    return out


def call(torch, plugin, Cn, B, F, H=4096, ld=K, phase=0, tail=False, sample_offset=0):
    """render_stft of a call with F frames into NaN-filled buffers: `out` with
    OUT_GUARD samples on either side, `mag` with one guard row before and after
    the F rows and its first row `phase` floats past a 16-byte boundary in
    channel 0 (the channel stride is a multiple of 4 floats).  Returns (out,
    mag, big_out, big_mag rows [Cn, F + 2, ld], result)."""
    L_ = (F - 1) * H + N + (17 if tail else 0)
    Lr = (L_ + B - 1) // B * B
    assert d.stft_frames(Lr, N, H) == F
    big_out = torch.full((Cn, Lr + 2 * OUT_GUARD), float("nan"), device="cuda")
    out = big_out[:, OUT_GUARD:OUT_GUARD + Lr]
    rows = (F + 2) * ld
    flat = torch.full((Cn, (rows + 4 + 3) // 4 * 4), float("nan"), device="cuda")
    assert flat.data_ptr() % 16 == 0
    # the first row (after the guard row) at `phase`
    start = (phase - ld) % 4
    big_mag = flat[:, start:start + rows].unflatten(1, (F + 2, ld))
    mag = big_mag[:, 1:F + 1, :]
    assert (mag.data_ptr() // 4) % 4 == phase
    file = torch.zeros((Cn, L_ + (L_ & 1)), device="cuda")
    o, m = d.render_stft(file, Cn, B, SR, plugin, H=H, ld=ld, out=out, mag=mag, sample_offset=sample_offset,
                         L_file=L_)
    res = last_result()
    torch.cuda.synchronize()
    assert m.shape == (Cn, F, K)
    return o, m, big_out, big_mag, res


def assert_same(torch, pair, Cn, B, F, **kw):
    name, reuse, every = pair
    what = (name, Cn, B, F, kw)
    o1, m1, bo1, bm1, r1 = call(torch, reuse, Cn, B, F, **kw)
    o2, m2, _, _, r2 = call(torch, every, Cn, B, F, **kw)
    assert r1 & L.DSP_RESULT_FRAME_REUSE, what
    assert not (r2 & L.DSP_RESULT_FRAME_REUSE), what
    assert torch.equal(m1, m2), what
    assert torch.equal(o1, o2), what
    # the render's guard samples are untouched
    assert bool(torch.isnan(bo1[:, :OUT_GUARD]).all()), what
    assert bool(torch.isnan(bo1[:, OUT_GUARD + o1.shape[1]:]).all()), what
    return bm1


@pytest.mark.parametrize("ld", [4097, 4098, 4099, 4100, 4101])
def test_every_phase_and_phase_step(torch_cuda, frame_run, plugins, ld):
    """One channel, B = 512, H = 4096, G = 4: every starting phase of the first
    row with every phase step per row (ld mod 4), over a single frame, a short
    run, one full run, a full run + 1 and two runs + a short one."""
    for F in (1, 3, 4, 5, 11):
        for phase in range(4):
            assert_same(torch_cuda, plugins[0], 1, 512, F, ld=ld, phase=phase)


@pytest.mark.parametrize("ld", [4097, 4100, 4104])
def test_no_stray_writes(torch_cuda, frame_run, plugins, ld):
    """NaN-filled buffers, one guard row before and after: every float outside
    [row, row + 4097) is still NaN -- the ld - K gap after each row and both
    guard rows -- and every float inside is finite (the head and tail dwords
    of a row's aligned pieces)."""
    torch = torch_cuda
    for F in (4, 11):
        for phase in range(4):
            _, m, _, big_mag, res = call(torch, plugins[0][1], 1, 512, F, ld=ld, phase=phase)
            what = (ld, F, phase)
            assert res & L.DSP_RESULT_FRAME_REUSE, what
            assert bool(torch.isfinite(m).all()), what
            assert bool(torch.isnan(big_mag[:, 0]).all()), what
            assert bool(torch.isnan(big_mag[:, F + 1]).all()), what
            if ld > K:
                assert bool(torch.isnan(big_mag[:, :, K:]).all()), what


# (Cn, B, H, tail, sample_offset / B)
SHAPES = [
    (3, 512, 4096, False, 0),   # channel groups
    (1, 128, 4096, False, 0),   # PER 1
    (2, 2048, 4096, False, 0),  # PER 16
    (2, 512, 2048, False, 0),   # two hops per row: the general render branch
    (2, 512, 4096, True, 0),    # a 17-sample tail (a partial tail wave)
    (2, 512, 4096, False, 7),   # sample_offset = 7 B
    (3, 256, 2048, True, 7),
]


@pytest.mark.parametrize("shape", SHAPES)
def test_other_shapes_on_the_path(torch_cuda, frame_run, plugins, shape):
    """The other instantiations and launch shapes, with the enum plugin and
    IR_test.cpp compiled unchanged: spectra, render and the render's guard
    samples as the every-frame call leaves them, no write outside the rows."""
    torch = torch_cuda
    Cn, B, H, tail, off = shape
    for pair in plugins:
        for F, ld, phase in ((5, 4097, 1), (11, 4100, 2)):
            big_mag = assert_same(torch, pair, Cn, B, F, H=H, ld=ld, phase=phase, tail=tail, sample_offset=off * B)
            assert bool(torch.isnan(big_mag[:, 0]).all()) and bool(torch.isnan(big_mag[:, F + 1]).all())
            assert bool(torch.isnan(big_mag[:, :, K:]).all())
