"""dspbench_render --loudness / --normalize LUFS / --true-peak-ceiling DBTP: the
render is measured with dsp_loudness (its written frames, every channel at
weight 1, true peak on), the result printed as one JSON line, and the render
scaled to the target level by one fp32 gain before the encode.  Without the
flags the output is byte for byte what it was."""
import numpy as np
import pytest

import dspbench as d
from cliutil import cuda as _cuda, json_line as _json_line, pcm16_file, run

FIELDS = ("integrated", "range", "momentary_max", "short_term_max", "sample_peak", "true_peak")

pytestmark = pytest.mark.gpu


def _pcm16(path, L=48_000, seed=51, amp=8000, spike=None, silent=False):
    def edit(raw):
        if silent:
            raw[:] = 0
        if spike is not None:
            raw[2 * spike] = 32700      # one near-full-scale sample on the left channel
    pcm16_file(path, 2, L, seed, lo=-amp, hi=amp + 1, edit=edit)
    return path


def _measure(torch, path):
    y, _ = d.wav.load(str(path))
    r = d.loudness(_cuda(torch, y), 48000)
    torch.cuda.synchronize()
    return r, np.asarray(y)


@pytest.mark.parametrize("extra", [("--loop", "4"), ("--world", "2")])
@pytest.mark.parametrize("flag", [("--loudness",), ("--normalize", "-23")])
def test_loudness_flags_exclude_other_modes(tmp_path, flag, extra):
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), *flag, *extra)
    assert r.returncode == 2 and "--loudness" in r.stderr


def test_ceiling_needs_normalize(tmp_path):
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "--true-peak-ceiling", "-1")
    assert r.returncode == 2 and "--normalize" in r.stderr


@pytest.mark.parametrize("flag,value", [("--true-peak-ceiling", "nan"), ("--true-peak-ceiling", "x"),
                                        ("--normalize", "inf"), ("--normalize", "-23dB")])
def test_level_arguments_must_be_finite_numbers(tmp_path, flag, value):
    args = ["--normalize", "-23", flag, value] if flag != "--normalize" else [flag, value]
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), *args)
    assert r.returncode == 2 and "usage" in r.stderr


def test_loudness_prints_the_measurement(torch_cuda, tmp_path):
    src, out = _pcm16(tmp_path / "in.wav"), tmp_path / "out.wav"
    r = run(str(src), str(out), "--plugin", "no_op", "--bits", "float", "--loudness")
    assert r.returncode == 0, r.stderr
    got = _json_line(r.stdout)
    want, y = _measure(torch_cuda, out)
    assert y.shape == (2, 94 * 512)
    for k in FIELDS:                  # (one second: no 3 s block, short_term_max is -inf on both sides)
        assert got[k] == want[k] or abs(got[k] - want[k]) <= 1e-9, (k, got[k], want[k])
    assert got["short_term_max"] == -np.inf and np.isfinite(got["integrated"])
    assert (got["blocks"], got["gated_blocks"]) == (want["blocks"], want["gated_blocks"]) and got["blocks"] == 7


def test_normalize_scales_the_render_by_one_gain(torch_cuda, tmp_path):
    src, a, b = _pcm16(tmp_path / "in.wav"), tmp_path / "a.wav", tmp_path / "b.wav"
    assert run(str(src), str(a), "--gain", "0.5", "--bits", "float").returncode == 0
    r = run(str(src), str(b), "--gain", "0.5", "--bits", "float", "--normalize", "-23", "--loudness")
    assert r.returncode == 0, r.stderr
    m, plain = _measure(torch_cuda, a)
    g = np.float32(10.0 ** ((-23.0 - m["integrated"]) / 20.0))
    assert _json_line(r.stdout)["gain"] == float(g)
    again, scaled = _measure(torch_cuda, b)
    assert np.array_equal(scaled, plain * g)              # one fp32 multiply per sample
    assert abs(again["integrated"] - -23.0) <= 1e-3


def test_true_peak_ceiling_lowers_the_gain(torch_cuda, tmp_path):
    src = _pcm16(tmp_path / "in.wav", amp=300, spike=20_000)
    a, b = tmp_path / "a.wav", tmp_path / "b.wav"
    assert run(str(src), str(a), "--plugin", "no_op", "--bits", "float").returncode == 0
    r = run(str(src), str(b), "--plugin", "no_op", "--bits", "float", "--normalize", "-23", "--true-peak-ceiling", "-1",
            "--loudness")
    assert r.returncode == 0, r.stderr
    m, plain = _measure(torch_cuda, a)
    limit = 10.0 ** (-1.0 / 20.0)
    g_level = np.float32(10.0 ** ((-23.0 - m["integrated"]) / 20.0))
    assert m["true_peak"] * float(g_level) > limit        # the level alone would pass the ceiling
    g = _json_line(r.stdout)["gain"]
    assert g < float(g_level) and g == float(np.float32(g))
    assert m["true_peak"] * g <= limit * (1 + 2.0 ** -22) and m["true_peak"] * g > limit * (1 - 1e-6)
    _, scaled = _measure(torch_cuda, b)
    assert np.array_equal(scaled, plain * np.float32(g))


def test_normalize_of_silence_is_an_error(tmp_path):
    src = _pcm16(tmp_path / "in.wav", silent=True)
    r = run(str(src), str(tmp_path / "out.wav"), "--normalize", "-23")
    assert r.returncode == 1 and "--normalize" in r.stderr
    assert not (tmp_path / "out.wav").exists()


def test_without_the_flags_nothing_changes(torch_cuda, tmp_path):
    """The same bytes as the Python face's render of the decoded samples,
    encoded by d.wav (the parent's output)."""
    src, out = _pcm16(tmp_path / "in.wav"), tmp_path / "out.wav"
    r = run(str(src), str(out), "--gain", "0.5", "--bits", "float")
    assert r.returncode == 0, r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    x, _ = d.wav.load(str(src))
    want = d.render_offline(_cuda(torch_cuda, x), 2, 512, 48000.0, d.Plugin.gain_test(0.5))
    torch_cuda.cuda.synchronize()
    got, info = d.wav.load(str(out))
    assert info.sample_rate == 48000 and np.array_equal(np.asarray(got), want.cpu().numpy())
    ref = tmp_path / "ref.wav"
    d.wav.save(str(ref), want.cpu().numpy(), 48000, fmt=3, bits=32)
    assert out.read_bytes() == ref.read_bytes()
