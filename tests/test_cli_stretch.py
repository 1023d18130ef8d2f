"""dspbench_render --stretch RATE and --pitch SEMITONES on a short WAV: the render
is stretched (dsp_time_stretch) or shifted (stretch, then dsp_resample) before
the encode; the JSON line's figures are the plans', and the output's length and
peak bin are right."""
import numpy as np
import pytest

import dspbench as d
import pvocutil as pu
from cliutil import cuda as _cuda, json_line, run

pytestmark = pytest.mark.gpu

N, K, H, K0 = 8192, 4097, 2048, 1000
LX = N + 8 * H  # 9 frames, 48 blocks of 512


def _tone(path):
    x = np.stack([pu.tones(LX, (K0,), (0.5,), (0.2,)), pu.tones(LX, (K0,), (0.25,), (1.1,))])
    d.wav.save(str(path), x, 48000)
    return x


def _peak_bins(torch, y):
    mag = d.stft_magnitude(_cuda(torch, y), 8192, H, d.DSP_WIN_HANN).cpu().numpy()[:, :, :K]
    return np.argmax(mag[:, 1:-1], axis=2)


def test_stretch(torch_cuda, tmp_path):
    x = _tone(tmp_path / "in.wav")
    out = tmp_path / "out.wav"
    r = run(str(tmp_path / "in.wav"), str(out), "--plugin", "no_op", "--stretch", "0.8")
    assert r.returncode == 0, r.stderr
    j = json_line(r.stdout)["stretch"]
    p = d.time_stretch_plan(LX, 0.8, 2, H)
    assert j == {"rate": 0.8, "p": 1, "q": 1, "hop": H, "frames_in": p["frames_in"], "frames_out": p["frames_out"],
                 "samples_in": LX, "samples_stretched": p["Lout"], "samples_out": p["Lout"]}
    got, info = d.wav.load(str(out))
    got = np.asarray(got)
    assert info.sample_rate == 48000 and got.shape == (2, p["Lout"])
    # the library's call on the same render, bit for bit; the tone stays in its bin
    want = d.time_stretch(_cuda(torch_cuda, x), 0.8, H).cpu().numpy()
    assert np.array_equal(got, want)
    assert np.all(_peak_bins(torch_cuda, got) == K0)


@pytest.mark.parametrize("semitones", [3, -2])
def test_pitch(torch_cuda, tmp_path, semitones):
    x = _tone(tmp_path / "in.wav")
    out = tmp_path / "out.wav"
    r = run(str(tmp_path / "in.wav"), str(out), "--plugin", "no_op", "--pitch", str(semitones), "--stretch-hop", str(H))
    assert r.returncode == 0, r.stderr
    j = json_line(r.stdout)["stretch"]
    pl = d.pitch_shift_plan(LX, semitones, 2, H)
    sp = d.time_stretch_plan(pl["padded"], pl["rate"], 2, H)
    assert j == {"rate": pl["rate"], "p": pl["p"], "q": pl["q"], "hop": H, "frames_in": sp["frames_in"],
                 "frames_out": sp["frames_out"], "samples_in": LX, "samples_stretched": pl["stretched"],
                 "samples_out": pl["Lout"]}
    got, _ = d.wav.load(str(out))
    got = np.asarray(got)
    assert got.shape == (2, pl["Lout"]) and abs(pl["Lout"] - LX) <= 1
    assert np.array_equal(got, d.pitch_shift(_cuda(torch_cuda, x), semitones, H).cpu().numpy())
    assert np.all(_peak_bins(torch_cuda, got) == round(K0 * pl["p"] / pl["q"]))


def test_stretch_then_levels(torch_cuda, tmp_path):
    """--normalize measures what is written: the stretched render."""
    _tone(tmp_path / "in.wav")
    out = tmp_path / "out.wav"
    r = run(str(tmp_path / "in.wav"), str(out), "--plugin", "no_op", "--stretch", "1.25", "--loudness")
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 2 and '"stretch"' in lines[0] and '"integrated"' in lines[1]
    got, _ = d.wav.load(str(out))
    assert np.asarray(got).shape[1] == d.time_stretch_plan(LX, 1.25, 2, H)["Lout"]


@pytest.mark.parametrize("extra", [("--deconvolve", "ref.wav"), ("--transfer", "ref.wav"), ("--stft", "m.f32"), ("--loop", "4")])
def test_stretch_excludes_other_modes(tmp_path, extra):
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "--stretch", "0.8", *extra)
    assert r.returncode == 2 and "--stretch" in r.stderr


def test_short_render_is_refused(torch_cuda, tmp_path):
    d.wav.save(str(tmp_path / "in.wav"), np.zeros((1, 4096), np.float32), 48000)
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "--plugin", "no_op", "--stretch", "0.8")
    assert r.returncode == 1 and "dsp_time_stretch_plan" in r.stderr
