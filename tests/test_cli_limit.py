"""dspbench_render --limit: with --normalize and --true-peak-ceiling the render
keeps the level it was asked for and a look-ahead limiter (dsp_limiter, true-peak
detector, linked) turns down only the milliseconds around each peak; without
--limit the whole programme is lowered until its loudest peak fits.

The file: 2 s of a -20 dBFS 1 kHz tone in stereo with three bursts of 1 ms at
0 dBFS (+20 dB on the tone) in its last 40 ms.  The float64 models
(limiterutil, loudnessutil) give for `--normalize -16 --true-peak-ceiling -1`:
with --limit -16.18 LUFS (the bursts' own energy and the release after them
are what is lost), without it -21.85 LUFS; a residual gain of 1 - 3e-8."""
import json

import numpy as np
import pytest

import dspbench as d
from cliutil import run
from wavutil import wav_image

SR = 48000

pytestmark = pytest.mark.gpu


def tone_with_bursts(path):
    n = np.arange(2 * SR)
    x = 0.1 * np.sin(2 * np.pi * 1000 * n / SR)
    for s in (1.96, 1.975, 1.99):
        i = int(s * SR)
        x[i:i + 48] = 0.999 * np.sin(2 * np.pi * 1000 * np.arange(48) / SR + np.pi / 2)
    raw = np.repeat(np.round(x * 32767.0).astype("<i2"), 2)  # stereo, interleaved
    path.write_bytes(wav_image(raw.tobytes(), fmt=1, channels=2, bits=16, sr=SR))
    return path


def measure(torch, path):
    y, _ = d.wav.load(str(path))
    r = d.loudness(torch.from_numpy(np.ascontiguousarray(np.asarray(y))).cuda(), SR)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("flags", [(), ("--normalize", "-16"), ("--true-peak-ceiling", "-1")])
def test_limit_needs_normalize_and_ceiling(tmp_path, flags):
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "--limit", *flags)
    assert r.returncode == 2 and ("--normalize" in r.stderr)


@pytest.mark.parametrize("extra", [("--loop", "4"), ("--world", "2")])
def test_limit_excludes_other_modes(tmp_path, extra):
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "--normalize", "-16", "--true-peak-ceiling", "-1",
            "--limit", *extra)
    assert r.returncode == 2 and "--limit" in r.stderr


def test_limit_holds_the_level(torch_cuda, tmp_path):
    src = tone_with_bursts(tmp_path / "in.wav")
    lim, low = tmp_path / "limited.wav", tmp_path / "lowered.wav"
    common = ("--plugin", "no_op", "--bits", "float", "--normalize", "-16", "--true-peak-ceiling", "-1")
    r = run(str(src), str(lim), *common, "--limit")
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])["limiter"]
    assert j["min_gain"] < 1.0 and j["limited"] > 0
    assert 0.89 < j["residual_gain"] <= 1.0  # (0.89 is 1 dB: a larger residue means the detector is wrong)
    got = measure(torch_cuda, lim)
    assert 20.0 * np.log10(got["true_peak"]) <= -1.0
    assert abs(got["integrated"] - -16.0) <= 0.5
    r = run(str(src), str(low), *common)
    assert r.returncode == 0, r.stderr
    lowered = measure(torch_cuda, low)
    assert 20.0 * np.log10(lowered["true_peak"]) <= -1.0 + 1e-4
    assert lowered["integrated"] < got["integrated"] - 3.0
