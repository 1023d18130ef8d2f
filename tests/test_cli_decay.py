"""dspbench_render --decay: the argument errors, the measurement loop closed
from the command line (--sweep, --convolve of a synthetic decaying impulse
response, --deconvolve ... --decay) and the stand-alone mode IR.wav --decay
OUT.csv, against tools/decay_model.py."""
import math

import numpy as np
import pytest

import dspbench as d
import decayutil as du
import decay_model as dm
from cliutil import json_line, run
from wavutil import wav_image

SR = 48000
COLUMNS = ["channel", "fm_hz", "edt_s", "t20_s", "t30_s", "c50_db", "c80_db", "d50", "ts_ms", "inr_db"]


def float_wav(path, x, sr=SR):
    x = np.atleast_2d(np.asarray(x, np.float32))
    path.write_bytes(wav_image(np.ascontiguousarray(x.T).astype("<f4").tobytes(), fmt=3, channels=x.shape[0], bits=32, sr=sr))
    return path


def read_wav(path):
    """(samples [C, L] float32, rate) of a float WAV, on the host."""
    image = np.fromfile(path, np.uint8)
    info = d.wav.parse(image)
    assert info.format == 3
    y = np.ascontiguousarray(d.wav.payload(image, info)).view("<f4")
    return np.ascontiguousarray(y.reshape(-1, info.channels).T), info.sample_rate


def read_csv(path):
    """[(channel, fm, {column: value or NaN})] of a --decay CSV."""
    lines = path.read_text().splitlines()
    assert lines[0].split(",") == COLUMNS
    rows = []
    for ln in lines[1:]:
        cells = ln.split(",")
        assert len(cells) == len(COLUMNS)
        rows.append((int(cells[0]), float(cells[1]), {k: (float(v) if v else math.nan) for k, v in zip(COLUMNS[2:], cells[2:])}))
    return rows


@pytest.mark.parametrize("extra", [("--plugin", "no_op"), ("--convolve", "ir.wav"), ("--loop", "4"), ("--stft", "m.f32"),
                                   ("--psd", "p.csv"), ("--rate", "44100"), ("--world", "2"),
                                   ("--comm-id", "id", "--stft", "m.f32")])
def test_decay_excludes_other_modes(tmp_path, extra):
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "--decay", str(tmp_path / "d.csv"), *extra)
    assert r.returncode == 2 and "--decay excludes" in r.stderr
    r = run(str(tmp_path / "in.wav"), "--decay", str(tmp_path / "d.csv"), *extra)
    assert r.returncode == 2 and "--decay excludes" in r.stderr


def test_decay_excludes_transfer(tmp_path):
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.csv"), "--transfer", "r.wav", "--decay", str(tmp_path / "d.csv"))
    assert r.returncode == 2 and "--decay excludes" in r.stderr


def test_decay_argument_errors(tmp_path):
    i, o, c = str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), str(tmp_path / "d.csv")
    r = run(i, o, "--decay", c)  # a render: neither --deconvolve nor alone
    assert r.returncode == 2 and "--decay goes with --deconvolve" in r.stderr
    r = run(i, o, "--decay-bands", "third")
    assert r.returncode == 2 and "--decay-bands needs --decay" in r.stderr
    r = run(i, "--decay", c, "--decay-bands", "fifth")
    assert r.returncode == 2 and "usage:" in r.stderr
    assert run(i, "--decay").returncode == 2 and run(i, o, "--deconvolve", "s.wav", "--decay").returncode == 2  # no value
    r = run(i, "--decay", c, "--loudness")
    assert r.returncode == 2 and "takes only --decay-bands and --device" in r.stderr
    r = run(i, "--decay", c, "--deconvolve", "s.wav")
    assert r.returncode == 2 and "takes only --decay-bands and --device" in r.stderr


def decaying_sine(T, L, f=1000.0):
    t = np.arange(L) / SR
    return (0.25 * np.exp(-3.0 * math.log(10.0) / T * t) * np.sin(2.0 * math.pi * f * t)).astype(np.float32)


def model_loop(s, h, pre, irl, eps=1e-6):
    """dsp_deconvolve's formula in float64 on sweep * h: the impulse response --deconvolve writes."""
    n = 1024
    while n < len(s) + len(h):
        n *= 2
    S = np.fft.rfft(s.astype(np.float64), n)
    Y = S * np.fft.rfft(h.astype(np.float64), n)
    lam = float(np.float32(eps)) * np.max(np.abs(S) ** 2)
    return np.roll(np.fft.irfft(Y * np.conj(S) / (np.abs(S) ** 2 + lam), n), pre)[:irl].astype(np.float32)


@pytest.mark.gpu
def test_sweep_convolve_deconvolve_decay_closes_the_loop(torch_cuda, tmp_path):
    """--sweep -> --convolve with a 1 kHz sine decaying with T = 0.3 s -> --deconvolve ...
    --decay: the CSV's T30 at 1 kHz within 2 % of T.  The float64 model of the same loop
    gives T30 = 0.3000 s (within 0.01 %, checked here to stay within 1 %), so 2 % stands."""
    T, Lh, pre, irl = 0.3, 24000, 100, 26000
    sweep = tmp_path / "sweep.wav"
    assert run("--sweep", "50:20000:1", str(sweep)).returncode == 0
    s = read_wav(sweep)[0][0]
    h = decaying_sine(T, Lh)
    played = float_wav(tmp_path / "played.wav", np.concatenate([s, np.zeros(Lh, np.float32)]))
    ir = float_wav(tmp_path / "room.wav", h)
    rec, got, csv = tmp_path / "recorded.wav", tmp_path / "measured_ir.wav", tmp_path / "decay.csv"
    r = run(str(played), str(rec), "--convolve", str(ir), "--bits", "float")
    assert r.returncode == 0, r.stderr
    r = run(str(rec), str(got), "--deconvolve", str(sweep), "--deconv-pre", str(pre), "--ir-length", str(irl),
            "--decay", str(csv))
    assert r.returncode == 0, r.stderr
    # the float64 model of the loop
    mir = model_loop(s, h, pre, irl)
    _, onset, e, m = dm.energies64(mir[None, :], SR, *du.OCTAVES)
    want = dm.derive(e[0, 5], m[0, 5], irl, int(onset[0]), 48, SR)
    print(f"model T30 at 1 kHz {want['t30']:.5f}")
    assert abs(want["t30"] - T) <= 0.01 * T
    rows = read_csv(csv)
    assert len(rows) == 10 and [c for c, _, _ in rows] == [0] * 10
    assert np.allclose([f for _, f, _ in rows], 1000.0 * dm.G ** np.arange(-5, 5), rtol=1e-8)
    v = rows[5][2]
    print(f"CLI T30 at 1 kHz {v['t30_s']:.5f}, T20 {v['t20_s']:.5f}, INR {v['inr_db']:.1f} dB")
    assert abs(v["t30_s"] - T) <= 0.02 * T
    assert abs(v["t20_s"] - T) <= 0.02 * T and v["inr_db"] >= 45.0
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 2  # --deconvolve's and --decay's
    j = json_line("\n".join(ln for ln in lines if "\"decay\"" in ln))["decay"]
    assert j["n"] == 65536 and j["hop"] == 48 and j["bands"] == 10 and j["fraction"] == 1
    y = read_wav(got)[0]
    assert y.shape == (1, irl)
    peak, on = dm.peak_onset(y[0])
    assert j["channels"] == [{"onset": on, "peak_dbfs": pytest.approx(20 * math.log10(peak), abs=1e-6)}]
    assert pre <= on <= pre + 3 and pre <= int(onset[0]) <= pre + 3  # the negative-time samples fall before the onset


@pytest.mark.gpu
@pytest.mark.parametrize("bands", ["octave", "third"])
def test_decay_of_a_file(torch_cuda, tmp_path, bands):
    """IR.wav --decay OUT.csv on the decaying sines, two channels at 44.1 kHz (the bands above
    22.05 kHz are left out): every row's channel and mid frequency, and in the three bands
    that hold a sine every cell against the float64 model's derive of the float64 energies --
    times within 1 %, C50 and C80 within 0.1 dB.  (The other bands hold leakage 100 dB down, where
    float32 and float64 differ by more than that.)"""
    sr = 44100
    h = dm.decaying_sines(sr)
    x = np.stack([h, 0.5 * h])
    src, csv = float_wav(tmp_path / "ir.wav", x, sr), tmp_path / "d.csv"
    r = run(str(src), "--decay", str(csv), *(("--decay-bands", "third") if bands == "third" else ()))
    assert r.returncode == 0, r.stderr
    spec = (1, -5, 3) if bands == "octave" else (3, -16, 12)
    _, onset, e, m = dm.energies64(x, sr, *spec)
    p = dm.plan(x.shape[1], sr, *spec)
    rows = read_csv(csv)
    assert len(rows) == 2 * p["bands"]
    j = json_line(r.stdout)["decay"]
    assert j["n"] == p["n"] and j["hop"] == 21 and j["bands"] == p["bands"] and j["fraction"] == spec[0]
    assert [c["onset"] for c in j["channels"]] == [38, 38]
    assert j["channels"][1]["peak_dbfs"] == pytest.approx(20 * math.log10(np.abs(x[1]).max()), abs=1e-6)
    for i, (c, fm, v) in enumerate(rows):
        b = i % p["bands"]
        assert c == i // p["bands"] and fm == pytest.approx(p["fm"][b], rel=1e-8)
        if not any(abs(fm - f) < 1.0 for f in (125.9, 1000.0, 7943.3)):
            continue
        want = dm.derive(e[c, b], m[c, b], x.shape[1], 38, 21, sr)
        assert want["flags"] == 0
        for col, key, tol in (("edt_s", "edt", None), ("t20_s", "t20", None), ("t30_s", "t30", None),
                              ("c50_db", "c50", 0.1), ("c80_db", "c80", 0.1)):
            if math.isnan(want[key]):
                assert math.isnan(v[col]), (fm, col)
            else:
                assert abs(v[col] - want[key]) <= (tol if tol else 0.01 * want[key]), (fm, col, v[col], want[key])
        # the noise tail of these clean sines is the arithmetic's own floor, 140 dB down in float32
        # and lower in float64: the INRs agree only in being far above every validity threshold
        assert min(v["inr_db"], want["inr"]) >= 80.0
        assert v["ts_ms"] == pytest.approx(1e3 * want["ts"], rel=0.01) and v["d50"] == pytest.approx(want["d50"], abs=0.01)
    if bands == "octave":
        for b, T in ((2, 1.0), (5, 0.6), (8, 0.3)):
            assert abs(rows[b][2]["t30_s"] - T) <= 0.01 * T
