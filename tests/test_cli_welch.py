"""dspbench_render --psd and --transfer: round trips on a 3-frame file against
the float64 model (tools/welch_model.py) within WELCH_TOL carried through the
derived figures, the JSON lines, and the refusals: what the options exclude,
files of different rates or lengths, and fewer samples than one frame."""
import numpy as np
import pytest

import welchutil as wu
import welch_model as wm
from cliutil import json_line, run
from wavutil import wav_image

SR, H = 48000, 4096
L3 = wu.N + 2 * H + 100  # three frames and a tail


def float_wav(path, x, sr=SR):
    x = np.atleast_2d(np.asarray(x, np.float32))
    path.write_bytes(wav_image(np.ascontiguousarray(x.T).astype("<f4").tobytes(), fmt=3, channels=x.shape[0], bits=32, sr=sr))
    return path


def read_csv(path, columns):
    lines = path.read_text().splitlines()
    head = lines[0].split(",")
    rows = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    assert len(head) == columns == rows.shape[1] and rows.shape[0] == wu.K and head[0] == "hz"
    assert np.allclose(rows[:, 0], np.arange(wu.K) * SR / wu.N, rtol=1e-8, atol=0)
    return head, rows


@pytest.mark.parametrize("args", [("--transfer", "r.wav", "--plugin", "no_op"), ("--transfer", "r.wav", "--psd", "p.csv"),
                                  ("--transfer", "r.wav", "--deconvolve", "s.wav"), ("--transfer", "r.wav", "--loudness"),
                                  ("--transfer", "r.wav", "--stft", "m.f32"), ("--transfer", "r.wav", "--world", "2"),
                                  ("--transfer", "r.wav", "--bits", "16")])
def test_transfer_excludes_other_modes(tmp_path, args):
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.csv"), *args)
    assert r.returncode == 2 and "--transfer excludes" in r.stderr


@pytest.mark.parametrize("args", [("--loop", "4"), ("--world", "2"), ("--comm-id", "id", "--stft", "m.f32")])
def test_psd_excludes_loop_and_multi_gpu(tmp_path, args):
    r = run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "--psd", str(tmp_path / "p.csv"), *args)
    assert r.returncode == 2 and "--psd excludes" in r.stderr
    assert run(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), "--psd").returncode == 2  # no value


@pytest.mark.gpu
def test_psd_round_trip(torch_cuda, tmp_path):
    """The average spectrum of a no_op render of three frames: 10 log10 of the one-sided
    density, within WELCH_TOL max(sxx) carried through the scale, and the JSON figures."""
    x, _ = wu.make_signals(L3, 2, seed=21)
    src, out, csv = float_wav(tmp_path / "in.wav", x), tmp_path / "out.wav", tmp_path / "psd.csv"
    r = run(str(src), str(out), "--plugin", "no_op", "--psd", str(csv))
    assert r.returncode == 0, r.stderr
    Lr = -(-L3 // 512) * 512  # the render: whole blocks, zeros past the file
    y = np.zeros((2, Lr), np.float32)
    y[:, :L3] = x
    sxx = wm.sums64(y, None, H, "hann")[0]
    w = wm.window_table("hann").astype(np.float64)
    g = np.full(wu.K, 2.0)
    g[0] = g[-1] = 1.0
    scale = g / (3 * SR * np.sum(w * w))
    want = sxx * scale
    head, rows = read_csv(csv, 3)
    assert head == ["hz", "ch0_db", "ch1_db"]
    got = 10.0 ** (rows[:, 1:].T / 10.0)
    for c in range(2):
        assert np.all(np.abs(got[c] - want[c]) <= wu.WELCH_TOL * sxx[c].max() * scale + 1e-7 * want[c])
    j = json_line(r.stdout)["psd"]
    assert j["frames"] == 3 and j["bins"] == wu.K and j["hop"] == H and len(j["channels"]) == 2
    for c, ch in enumerate(j["channels"]):
        at = int(np.argmax(rows[:, 1 + c]))
        assert ch["peak_hz"] == pytest.approx(at * SR / wu.N) and ch["peak_db"] == pytest.approx(rows[at, 1 + c], abs=1e-6)
        assert ch["power_db"] == pytest.approx(10 * np.log10(np.sum(want[c]) * SR / wu.N), abs=1e-4)
    assert out.exists()


@pytest.mark.gpu
def test_transfer_round_trip(torch_cuda, tmp_path):
    """|H1| in dB, its phase and the coherence of a 2-channel recording against a mono
    reference, three frames: the float64 model's, within WELCH_TOL carried through the
    quotients (first order, the sums' errors relative to each row's maximum)."""
    x, ref = wu.make_signals(L3, 2, seed=22)
    rec, rf, csv = float_wav(tmp_path / "rec.wav", x), float_wav(tmp_path / "ref.wav", ref), tmp_path / "h.csv"
    r = run(str(rec), str(csv), "--transfer", str(rf))
    assert r.returncode == 0, r.stderr
    sxx, srr, sxy = wm.sums64(x, ref, H, "hann")
    head, rows = read_csv(csv, 7)
    assert head == ["hz", "ch0_h1_db", "ch0_phase_rad", "ch0_coherence", "ch1_h1_db", "ch1_phase_rad", "ch1_coherence"]
    T = wu.WELCH_TOL
    cohs = []
    for c in range(2):
        Hs = sxy[c] / srr
        got = 10.0 ** (rows[:, 1 + 3 * c] / 20.0) * np.exp(1j * rows[:, 2 + 3 * c])
        mx, mr = sxx[c].max(), srr.max()
        bound = T * (np.sqrt(mx * mr) + np.abs(Hs) * mr) / srr * 1.01 + 1e-7 * np.abs(Hs)
        assert np.all(np.abs(got - Hs) <= bound)
        coh = np.abs(sxy[c]) ** 2 / (sxx[c] * srr)
        cb = coh * T * (2 * np.sqrt(mx * mr) / np.abs(sxy[c]) + mx / sxx[c] + mr / srr) * 1.01 + 1e-8
        assert np.all(np.abs(rows[:, 3 + 3 * c] - coh) <= cb)
        assert np.all(rows[:, 3 + 3 * c] > 0) and np.all(rows[:, 3 + 3 * c] <= 1 + cb)
        cohs.append(coh)
    j = json_line(r.stdout)["transfer"]
    assert j["frames"] == 3 and j["bins"] == wu.K and j["hop"] == H and len(j["channels"]) == 2
    for c, ch in enumerate(j["channels"]):
        assert ch["mean_coherence"] == pytest.approx(np.mean(cohs[c]), abs=1e-5)
        assert ch["min_coherence"] == pytest.approx(np.min(cohs[c]), abs=1e-5)
        assert ch["gain_db"] == pytest.approx(10 * np.log10(np.sum(sxx[c]) / np.sum(srr)), abs=1e-4)


@pytest.mark.gpu
def test_transfer_refuses_rates_lengths_and_short_files(torch_cuda, tmp_path):
    x, ref = wu.make_signals(L3, 1, seed=23)
    rec = float_wav(tmp_path / "rec.wav", x)
    out = tmp_path / "h.csv"
    r = run(str(rec), str(out), "--transfer", str(float_wav(tmp_path / "r441.wav", ref, 44100)))
    assert r.returncode == 1 and "Hz" in r.stderr and not out.exists()
    r = run(str(rec), str(out), "--transfer", str(float_wav(tmp_path / "rshort.wav", ref[:-1])))
    assert r.returncode == 1 and "frames" in r.stderr and not out.exists()
    short = float_wav(tmp_path / "short.wav", x[:, :wu.N - 1])
    r = run(str(short), str(out), "--transfer", str(float_wav(tmp_path / "rs.wav", ref[:wu.N - 1])))
    assert r.returncode == 1 and "fewer than one" in r.stderr and not out.exists()


@pytest.mark.gpu
def test_psd_refuses_a_render_shorter_than_a_frame(torch_cuda, tmp_path):
    x, _ = wu.make_signals(wu.N - 512, 1, seed=24)  # 15 blocks of 512: 7680 < 8192
    out, csv = tmp_path / "o.wav", tmp_path / "p.csv"
    r = run(str(float_wav(tmp_path / "in.wav", x)), str(out), "--psd", str(csv))
    assert r.returncode == 1 and "fewer than one" in r.stderr and not csv.exists() and not out.exists()
