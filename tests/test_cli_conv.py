"""dspbench_render --convolve IR.wav: the command line's DSP_PLUGIN_CONV path.
The IR file goes through the same parse + GPU decode as the input, its first
channel is the taps; the written file equals the Python face's render of the
decoded input with those taps bit for bit.  --convolve with --plugin is a
usage error (exit 2, no GPU touched)."""
import numpy as np
import pytest

import dspbench as d
from cliutil import pcm16_file, run, split_chunks

pytestmark = pytest.mark.gpu


def _pcm16(path, channels, L, seed, **image):
    pcm16_file(path, channels, L, seed, **image)
    return path


def test_convolve_and_plugin_exclude_each_other(tmp_path):
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "--convolve", str(tmp_path / "ir.wav"),
            "--plugin", "no_op")
    assert r.returncode == 2 and "--convolve" in r.stderr


def test_convolve_file_matches_python_render(torch_cuda, tmp_path):
    src = _pcm16(tmp_path / "in.wav", 2, 48_000 * 3, 21)
    irp = _pcm16(tmp_path / "ir.wav", 2, 6000, 22)   # stereo IR: the first channel is the taps
    out = tmp_path / "out.wav"
    r = run(str(src), str(out), "--convolve", str(irp), "--block", "512", "--bits", "float")
    assert r.returncode == 0, r.stderr
    got, info = d.wav.load(str(out))
    assert info.format == 3 and info.bits_per_sample == 32
    x, _ = d.wav.load(str(src))
    ir, _ = d.wav.load(str(irp))
    taps = np.ascontiguousarray(np.asarray(ir)[0])
    assert taps.size == 6000
    want = d.render_offline(torch_cuda.from_numpy(np.ascontiguousarray(np.asarray(x))).cuda(), 2, 512, 48000.0,
                            d.Plugin.conv(taps))
    torch_cuda.cuda.synchronize()
    want = want.cpu().numpy()
    got = np.asarray(got)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_response_split_over_two_data_chunks(torch_cuda, tmp_path):
    """--convolve reads its file through the input's loader: a 257-tap response
    in two data chunks, an odd-sized unrelated chunk between them, gives the
    bytes of the same taps in one chunk."""
    src = _pcm16(tmp_path / "in.wav", 2, 3001, 23)
    one = _pcm16(tmp_path / "ir_one.wav", 1, 257, 24)
    two = _pcm16(tmp_path / "ir_two.wav", 1, 257, 24, **split_chunks(2 * 257, 2 * 100))
    assert len(two.read_bytes()) == len(one.read_bytes()) + 8 + 8 + 6
    outs = []
    for ir in (one, two):
        outs.append(tmp_path / ("out_" + ir.name))
        r = run(str(src), str(outs[-1]), "--convolve", str(ir), "--block", "256", "--bits", "float")
        assert r.returncode == 0, r.stderr
    assert outs[0].read_bytes() == outs[1].read_bytes() and len(outs[0].read_bytes()) == 46 + 12 * 256 * 8
