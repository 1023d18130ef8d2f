"""dspbench_render --sweep and --deconvolve: the measurement loop from the
command line.  --sweep writes dspbench.sweep's samples bit for bit without
opening a device; the chain sweep -> --convolve KNOWN_IR.wav -> --deconvolve
SWEEP.wav gives the known band-limited response back within the float64
model's recorded margin (deconvutil.RECOVERY_TOL) plus the device's DEC_TOL."""
import json
import os

import numpy as np
import pytest

import dspbench as d
import deconvutil as du
from cliutil import run, split_chunks
from wavutil import wav_image

S = du.SWEEP  # what `--sweep 50:20000:0.5` writes: amplitude 0.5, 10 ms fades, 48 kHz


def float_wav(path, x, sr=48000):
    """x [C, L] float32 as a float WAV."""
    x = np.atleast_2d(np.asarray(x, np.float32))
    path.write_bytes(wav_image(np.ascontiguousarray(x.T).astype("<f4").tobytes(), fmt=3, channels=x.shape[0], bits=32, sr=sr))
    return path


def read_wav(path):
    """(samples [C, L] float32, rate) of a float or 16-bit WAV, on the host."""
    image = np.fromfile(path, np.uint8)
    info = d.wav.parse(image)
    pay = np.ascontiguousarray(d.wav.payload(image, info))
    if info.format == 3:
        y = pay.view("<f4")
    else:
        assert info.bits_per_sample == 16
        y = (pay.view("<i2") / np.float32(32768.0)).astype(np.float32)
    return np.ascontiguousarray(y.reshape(-1, info.channels).T), info.sample_rate


@pytest.mark.parametrize("order", ["spec_first", "out_first"])
def test_sweep_is_dsp_sweep_bit_for_bit_without_a_device(tmp_path, order):
    out = tmp_path / "sweep.wav"
    args = ("--sweep", "50:20000:0.5", str(out)) if order == "spec_first" else (str(out), "--sweep", "50:20000:0.5")
    # no device is visible to the process: the mode never opens one
    r = run(*args, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr
    y, sr = read_wav(out)
    want = d.sweep(S["sr"], S["f1"], S["f2"], S["seconds"], S["amplitude"], S["fade"])
    assert sr == 48000 and y.shape == (1, want.size) and y.dtype == np.float32
    assert np.array_equal(y[0].view(np.int32), want.view(np.int32))


def test_sweep_rate_and_bits(tmp_path):
    out = tmp_path / "s16.wav"
    r = run("--sweep", "100:8000:0.1:44100:16", str(out))
    assert r.returncode == 0, r.stderr
    y, sr = read_wav(out)
    want = d.sweep(44100, 100.0, 8000.0, 0.1, 0.5, 441)
    assert sr == 44100 and y.shape == (1, 4410) and np.max(np.abs(y[0] - want)) <= 2.0 ** -16


@pytest.mark.parametrize("args", [("--sweep", "50:20000"), ("--sweep", "50:20000:0.5:48000:12"), ("--sweep", "0:100:1"),
                                  ("--sweep", "50:20000:0.5", "--bits", "16")])
def test_sweep_bad_arguments(tmp_path, args):
    r = run(*args, str(tmp_path / "o.wav"))
    assert r.returncode != 0 and not (tmp_path / "o.wav").exists()


@pytest.mark.parametrize("extra", [("--plugin", "no_op"), ("--convolve", "ir.wav"), ("--loop", "4"), ("--normalize", "-16"),
                                   ("--world", "2"), ("--comm-id", "id")])
def test_deconvolve_excludes_other_modes(tmp_path, extra):
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "--deconvolve", str(tmp_path / "ref.wav"), *extra)
    assert r.returncode == 2 and "--deconvolve" in r.stderr


def test_deconv_options_need_deconvolve(tmp_path):
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "--deconv-pre", "5")
    assert r.returncode == 2 and "--deconvolve" in r.stderr


@pytest.mark.gpu
def test_rate_mismatch_is_an_error(torch_cuda, tmp_path):
    a = float_wav(tmp_path / "a.wav", np.ones((1, 2000)), 48000)
    b = float_wav(tmp_path / "b.wav", np.ones((1, 2000)), 44100)
    r = run(str(a), str(tmp_path / "o.wav"), "--deconvolve", str(b))
    assert r.returncode == 1 and "Hz" in r.stderr and not (tmp_path / "o.wav").exists()


@pytest.mark.gpu
def test_sweep_convolve_deconvolve_recovers_the_response(torch_cuda, tmp_path):
    sweep = tmp_path / "sweep.wav"
    assert run("--sweep", "50:20000:0.5", str(sweep)).returncode == 0
    x = read_wav(sweep)[0][0]
    # what is played: the sweep and 2048 samples of silence for the response's tail, on two channels
    played = float_wav(tmp_path / "played.wav", np.stack([np.concatenate([x, np.zeros(2048, np.float32)])] * 2))
    h = du.bandpass_ir(L=1024)
    ir = float_wav(tmp_path / "known_ir.wav", h)
    rec, got = tmp_path / "recorded.wav", tmp_path / "measured_ir.wav"
    r = run(str(played), str(rec), "--convolve", str(ir), "--bits", "float")
    assert r.returncode == 0, r.stderr
    pre = 100
    r = run(str(rec), str(got), "--deconvolve", str(sweep), "--deconv-pre", str(pre), "--ir-length", "4096")
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n"] == 32768 and j["eps"] == 1e-6 and j["pre"] == pre and j["ir_length"] == 4096 and len(j["peaks"]) == 2
    y, sr = read_wav(got)
    assert sr == 48000 and y.shape == (2, 4096) and y.dtype == np.float32
    want = np.zeros(4096)
    want[pre:pre + 1024] = h
    at = int(np.argmax(np.abs(want)))
    for c in range(2):
        err = np.max(np.abs(y[c] - want)) / np.max(np.abs(want))
        print(f"channel {c}: recovery {err:.3e}")
        assert err <= du.RECOVERY_TOL + du.DEC_TOL
        assert j["peaks"][c]["index"] == at == int(np.argmax(np.abs(y[c])))
        assert j["peaks"][c]["value"] == float(y[c, at])
    # the default length: min(n, 2^20), directly usable by --convolve
    r = run(str(rec), str(got), "--deconvolve", str(sweep))
    assert r.returncode == 0, r.stderr
    assert read_wav(got)[0].shape == (2, 32768)
    r = run(str(played), str(tmp_path / "again.wav"), "--convolve", str(got), "--bits", "float")
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_excitation_split_over_two_data_chunks(torch_cuda, tmp_path):
    """--deconvolve reads its file through the input's loader: a 0.05 s sweep in
    two data chunks, an odd-sized unrelated chunk between them, gives the bytes
    (and the JSON line) of the same sweep in one chunk."""
    sweep = tmp_path / "sweep.wav"
    assert run("--sweep", "50:20000:0.05", str(sweep)).returncode == 0
    x = read_wav(sweep)[0]
    assert x.shape == (1, 2400)
    data = x[0].astype("<f4").tobytes()
    one, two = tmp_path / "ref_one.wav", tmp_path / "ref_two.wav"
    one.write_bytes(wav_image(data, fmt=3, channels=1, bits=32))
    two.write_bytes(wav_image(data, fmt=3, channels=1, bits=32, **split_chunks(len(data), 4 * 1001)))
    assert len(two.read_bytes()) == len(one.read_bytes()) + 8 + 8 + 6
    outs, lines = [], []
    for ref in (one, two):
        outs.append(tmp_path / ("ir_" + ref.name))
        r = run(str(sweep), str(outs[-1]), "--deconvolve", str(ref))
        assert r.returncode == 0, r.stderr
        lines.append([ln for ln in r.stdout.splitlines() if ln.startswith("{")])
    assert outs[0].read_bytes() == outs[1].read_bytes() and lines[0] == lines[1] and len(lines[0]) == 1
    assert read_wav(outs[0])[0].shape[0] == 1
