"""Frame reuse in the fused IR_test render + STFT (stft_pk PER path).

With H % B == 0 every frame of a call holds the same samples, so a wave
computes the spectrum once and stores it for a run of G frames
(DSP_RESULT_FRAME_REUSE); DSP_EXEC_EVERY_FRAME keeps one FFT per frame.  Both
run the same instruction sequence on the same inputs, so the outputs are
compared bit for bit.  The library picks G from the call's length (1 for a
call too short to fill the device), so the small shapes here set it through
the DSP_DEBUG_FRAME_RUN hook; one test runs a call long enough for the
library's own choice.
"""
import os

import numpy as np
import pytest

import dspbench as d
import dspbench._lib as L
from dspbench.api import last_result

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
IR_CO = os.path.join(os.path.dirname(HERE), "dsp-bench_amd", "modules", "mod_IR_test.co")
PEAK_REL_TOL = 1e-6
N = 8192
G = 5  # frames per wave in these tests (the hook)
SR = 48000.0


@pytest.fixture
def frame_run():
    """Sets the frames per wave for the test and restores the library's choice."""
    def set_run(g):
        L.check(L.lib().dsp_debug_set(L.DSP_DEBUG_FRAME_RUN, g), "dsp_debug_set")
    set_run(G)
    yield set_run
    set_run(0)


@pytest.fixture(scope="module")
def plugins():
    """(name, plugin with reuse, plugin with every frame): the enum kind and,
    where it is built, IR_test.cpp compiled unchanged (its table class)."""
    out = [("enum", d.Plugin.ir_test(), d.Plugin.ir_test(every_frame=True))]
    if os.path.exists(IR_CO):
        with open(IR_CO, "rb") as f:
            mod = d.module.Module(f.read())
        params = mod.default_parameters()
        mod.initialize_state(params, 3, SR)
        out.append(("source", mod.plugin(params, "IR_test"), mod.plugin(params, "IR_test", every_frame=True)))
    return out


def length(F, H, B, tail):
    """A file length that gives F frames: blocks up to (F - 1) H + N exactly
    (then [F H, Lr) is the N - H overlap, whole hops), or 17 samples more (one
    more block: a partial tail wave; H = N: the only tail)."""
    return (F - 1) * H + N + (17 if tail else 0)


def call(torch, plugin, Cn, B, L_, H=4096, ld=4097, sample_offset=0, guard=0):
    """render_stft into fresh NaN-filled buffers; returns (out view, mag view,
    the whole buffers, result)."""
    nb = (L_ + B - 1) // B
    Lr = nb * B
    F = d.stft_frames(Lr, N, H)
    big_out = torch.full((Cn, Lr + 2 * guard), float("nan"), device="cuda")
    big_mag = torch.full((Cn, F + 2 * (1 if guard else 0), ld), float("nan"), device="cuda")
    out = big_out[:, guard:guard + Lr]
    mag = big_mag[:, (1 if guard else 0):(1 if guard else 0) + F, :]
    # (rows of an even stride: the fused launch needs 8-byte aligned rows)
    file = torch.zeros((Cn, L_ + (L_ & 1)), device="cuda")
    o, m = d.render_stft(file, Cn, B, SR, plugin, H=H, ld=ld, out=out, mag=mag, sample_offset=sample_offset,
                         L_file=L_)
    res = last_result()
    torch.cuda.synchronize()
    return o, m, big_out, big_mag, res


def assert_same(torch, B, Cn, F, H, plugin_pair, tail, off, ld):
    name, reuse, every = plugin_pair
    L_ = length(F, H, B, tail)
    what = (name, B, Cn, F, H, tail, off, ld)
    o1, m1, _, _, r1 = call(torch, reuse, Cn, B, L_, H, ld, off)
    o2, m2, _, _, r2 = call(torch, every, Cn, B, L_, H, ld, off)
    assert m1.shape[1] == F, what
    assert r1 & L.DSP_RESULT_FRAME_REUSE, what
    assert not (r2 & L.DSP_RESULT_FRAME_REUSE), what
    assert torch.equal(o1, o2), what
    assert torch.equal(m1, m2), what
    return o1, m1


# every (tail, sample_offset / B, ld) value with every other, over the F values
COMBOS = [(False, 0, 4097), (True, 7, 4100), (True, 0, 4100), (False, 7, 4097)]


@pytest.mark.parametrize("Cn", [1, 2, 3])
@pytest.mark.parametrize("B", [128, 256, 512, 2048])
def test_reuse_is_bit_identical_to_every_frame(torch_cuda, frame_run, plugins, B, Cn):
    """PER 1, 2, 4, 16 at the headline hop: runs of G frames with a short last
    run (F = G - 1, G + 1, 2 G + 3), one run (F = G) and one frame."""
    for pair in plugins:
        for F in (1, G - 1, G, G + 1, 2 * G + 3):
            for tail, off, ld in COMBOS:
                assert_same(torch_cuda, B, Cn, F, 4096, pair, tail, off * B, ld)


@pytest.mark.parametrize("H", [2048, 8192])
def test_other_invariant_hops(torch_cuda, oracle, frame_run, plugins, H):
    """H = 2048 (the general store branch) and H = N, B = 512: the same
    comparison, and the spectra within 1e-6 of the peak of float64."""
    B, Cn = 512, 2
    for pair in plugins:
        for F in (G + 1, 2 * G + 3):
            for tail in (False, True):
                o1, m1 = assert_same(torch_cuda, B, Cn, F, H, pair, tail, 0, 4097)
                L_ = length(F, H, B, tail)
                ref = oracle.render_offline([np.zeros(L_, np.float32)] * Cn, Cn, B, SR,
                                            oracle.restated_plugin("IR_test"))
                assert np.array_equal(o1.cpu().numpy(), ref)
                m64 = oracle.np_stft_mag(ref[0], N, H, oracle.WIN_HANN, 4097)
                for c in range(Cn):
                    mm = m1[c].cpu().numpy().astype(np.float64)
                    err = float(np.max(np.abs(mm - m64).max(axis=1) / m64.max(axis=1)))
                    assert err <= PEAK_REL_TOL, (H, F, tail, c, err)


def test_non_invariant_hop_stays_per_frame(torch_cuda, oracle, frame_run):
    """B = 512, H = 4224 (a multiple of 128, not of 512): the frames differ, so
    no reuse whatever the hook says; render bit-exact, spectra within 1e-6."""
    B, H, Cn, F = 512, 4224, 2, 2 * G + 3
    L_ = length(F, H, B, True)
    o1, m1, _, _, res = call(torch_cuda, d.Plugin.ir_test(), Cn, B, L_, H)
    assert not (res & L.DSP_RESULT_FRAME_REUSE)
    ref = oracle.render_offline([np.zeros(L_, np.float32)] * Cn, Cn, B, SR, oracle.restated_plugin("IR_test"))
    assert np.array_equal(o1.cpu().numpy(), ref)
    m64 = oracle.np_stft_mag(ref[0], N, H, oracle.WIN_HANN, 4097)
    assert m1.shape[1] == m64.shape[0]
    for c in range(Cn):
        mm = m1[c].cpu().numpy().astype(np.float64)
        err = float(np.max(np.abs(mm - m64).max(axis=1) / m64.max(axis=1)))
        assert err <= PEAK_REL_TOL, (c, err)


@pytest.mark.parametrize("ld", [4097, 4100])
@pytest.mark.parametrize("H", [4096, 2048])
def test_no_write_outside_a_run(torch_cuda, frame_run, H, ld):
    """out and mag are views into NaN-filled buffers: after the call the guard
    samples around each channel's render, the guard rows around its spectra
    and the columns between K and ld are still NaN, and nothing inside is."""
    torch = torch_cuda
    B, Cn, guard = 512, 3, 4098
    for F in (1, G, 2 * G + 3):
        for tail in (False, True):
            o, m, big_out, big_mag, res = call(torch, d.Plugin.ir_test(), Cn, B, length(F, H, B, tail), H, ld,
                                               guard=guard)
            assert res & L.DSP_RESULT_FRAME_REUSE
            assert not bool(torch.isnan(o).any())
            assert not bool(torch.isnan(m).any())
            assert bool(torch.isnan(big_out[:, :guard]).all()) and bool(torch.isnan(big_out[:, guard + o.shape[1]:]).all())
            assert bool(torch.isnan(big_mag[:, 0]).all()) and bool(torch.isnan(big_mag[:, F + 1]).all())
            if ld > 4097:
                assert bool(torch.isnan(big_mag[:, :, 4097:]).all())


def test_chunked_driver_passes_the_flag_on(torch_cuda, frame_run):
    """render_stft_host over a few chunks: DSP_EXEC_EVERY_FRAME reaches every
    chunk (the result bit follows it) and the rows are the same."""
    B, Cn = 512, 2
    x = np.zeros((Cn, 40 * 4096 + 300), np.float32)
    o1, m1 = d.render_stft_host(x, Cn, B, SR, d.Plugin.ir_test(), chunk=1 << 15)
    assert last_result() & L.DSP_RESULT_FRAME_REUSE
    o2, m2 = d.render_stft_host(x, Cn, B, SR, d.Plugin.ir_test(every_frame=True), chunk=1 << 15)
    assert not (last_result() & L.DSP_RESULT_FRAME_REUSE)
    assert np.array_equal(o1, o2) and np.array_equal(m1, m2)
    assert not np.isnan(m1).any()


def test_library_choice_of_run(torch_cuda, frame_run):
    """Without the hook: a short call keeps one frame per wave (bit clear), a
    call with more frames than the device has wave slots reuses (bit set) and
    matches the every-frame call bit for bit."""
    torch = torch_cuda
    frame_run(0)
    B, Cn = 512, 3
    _, _, _, _, res = call(torch, d.Plugin.ir_test(), Cn, B, length(9, 4096, B, True))
    assert not (res & L.DSP_RESULT_FRAME_REUSE)
    F = 1500  # 3 channels x 1500 frames > 2048 resident waves
    L_ = length(F, 4096, B, True)
    o1, m1, _, _, r1 = call(torch, d.Plugin.ir_test(), Cn, B, L_)
    o2, m2, _, _, r2 = call(torch, d.Plugin.ir_test(every_frame=True), Cn, B, L_)
    assert r1 & L.DSP_RESULT_FRAME_REUSE and not (r2 & L.DSP_RESULT_FRAME_REUSE)
    assert torch.equal(o1, o2) and torch.equal(m1, m2)
