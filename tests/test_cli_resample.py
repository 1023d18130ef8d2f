"""dspbench_render --rate R: the input is converted from its header's rate to R
on the GPU before the render (dsp_resample, default quality), R goes to the
plugin and into the output header; with --convolve the impulse response is
converted from its own rate and scaled by ir_rate / R.  Without --rate the
output is byte for byte what it was."""
import numpy as np
import pytest

import dspbench as d
from cliutil import cuda as _cuda, pcm16_file, run

pytestmark = pytest.mark.gpu


def _pcm16(path, channels, L, seed, rate):
    pcm16_file(path, channels, L, seed, sr=rate)
    return path


@pytest.mark.parametrize("extra", [("--device-rate", "48000"), ("--loop", "4"), ("--world", "2")])
def test_rate_excludes_other_modes(tmp_path, extra):
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "--rate", "48000", *extra)
    assert r.returncode == 2 and "--rate" in r.stderr


def test_rate_converts_the_input(torch_cuda, tmp_path):
    src = _pcm16(tmp_path / "in.wav", 2, 30_000, 31, 44100)
    out = tmp_path / "out.wav"
    r = run(str(src), str(out), "--rate", "48000", "--plugin", "no_op", "--block", "512", "--bits", "float")
    assert r.returncode == 0, r.stderr
    got, info = d.wav.load(str(out))
    assert info.sample_rate == 48000 and info.format == 3
    x, xi = d.wav.load(str(src))
    assert xi.sample_rate == 44100
    want = d.resample(_cuda(torch_cuda, x), 44100, 48000)
    torch_cuda.cuda.synchronize()
    want = want.cpu().numpy()
    got = np.asarray(got)
    Lout = want.shape[1]
    assert Lout == d.resample_plan(44100, 48000, 30_000)["Lout"] and got.shape[1] == -(-Lout // 512) * 512
    assert np.array_equal(got[:, :Lout], want) and not got[:, Lout:].any()


def test_rate_converts_the_impulse_response(torch_cuda, tmp_path):
    src = _pcm16(tmp_path / "in.wav", 2, 30_000, 32, 48000)     # already at the target rate
    irp = _pcm16(tmp_path / "ir.wav", 1, 6000, 33, 44100)
    out = tmp_path / "out.wav"
    r = run(str(src), str(out), "--convolve", str(irp), "--rate", "48000", "--block", "512", "--bits", "float")
    assert r.returncode == 0, r.stderr
    got, info = d.wav.load(str(out))
    assert info.sample_rate == 48000
    x, _ = d.wav.load(str(src))
    ir, _ = d.wav.load(str(irp))
    taps = d.resample(_cuda(torch_cuda, np.asarray(ir)[:1]), 44100, 48000)
    torch_cuda.cuda.synchronize()
    taps = taps.cpu().numpy()[0] * np.float32(44100 / 48000)
    assert taps.dtype == np.float32 and taps.size == d.resample_plan(44100, 48000, 6000)["Lout"]
    want = d.render_offline(_cuda(torch_cuda, x), 2, 512, 48000.0, d.Plugin.conv(taps))
    torch_cuda.cuda.synchronize()
    assert np.array_equal(np.asarray(got), want.cpu().numpy())


def test_without_rate_nothing_changes(torch_cuda, tmp_path):
    """The file's rate is carried, not applied: the same bytes as the Python
    face's render of the decoded samples, header rate the input's."""
    src = _pcm16(tmp_path / "in.wav", 2, 30_000, 34, 44100)
    a, b = tmp_path / "a.wav", tmp_path / "b.wav"
    assert run(str(src), str(a), "--gain", "0.5", "--bits", "float").returncode == 0
    assert run(str(src), str(b), "--gain", "0.5", "--bits", "float", "--rate", "44100").returncode == 0
    assert a.read_bytes() == b.read_bytes()       # --rate equal to the file's: no conversion either
    got, info = d.wav.load(str(a))
    assert info.sample_rate == 44100
    x, _ = d.wav.load(str(src))
    want = d.render_offline(_cuda(torch_cuda, x), 2, 512, 44100.0, d.Plugin.gain_test(0.5))
    torch_cuda.cuda.synchronize()
    assert np.array_equal(np.asarray(got), want.cpu().numpy())
