"""dsp_decay's host half (decay_host.cpp) against tools/decay_model.py: the plan,
dsp_decay_derive on the model's energies, its validity flags, the silent and
the short row, the result's layout, and the known-answer impulse response
through the float64 model."""
import ctypes as C
import math

import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L_
import decayutil  # noqa: F401  (puts tools/ on the path)
import decay_model as dm

FIELDS = ("edt", "t20", "t30", "c50", "c80", "d50", "ts", "inr")


@pytest.mark.parametrize("sr,hop", [(48000, 48), (44100, 21), (96000, 96), (88200, 63), (32000, 32)])
def test_hop(sr, hop):
    p = d.decay_plan(1000, sr, 1, 0, 0)
    assert p["hop"] == hop == dm.hop_of(sr)
    assert (sr // 100) % hop == 0 and hop <= sr // 1000
    assert p["hops"] == -(-1000 // hop) + 1


def status(L, sr, fraction, k_lo, k_hi, C_=1):
    sp = L_.dsp_decay_spec(fraction, k_lo, k_hi)
    return L_.lib().dsp_decay_plan(L, C_, sr, C.byref(sp), None, None, None, None, None, None, None)


def test_plan_refusals():
    assert status(1000, 22050, 1, 0, 0) == L_.DSP_ERR_UNSUPPORTED  # 22050 % 100 != 0
    assert status(1000, 48000, 1, 0, 0) == L_.DSP_OK
    assert status(0, 48000, 1, 0, 0) == L_.DSP_ERR_INVALID
    assert status(1000, 48000, 1, 0, 0, C_=0) == L_.DSP_ERR_INVALID
    assert status(1000, 48000, 2, 0, 0) == L_.DSP_ERR_INVALID
    assert status(1000, 48000, 1, 1, 0) == L_.DSP_ERR_INVALID
    assert status(1000, 48000, 3, -16, 16) == L_.DSP_ERR_INVALID  # 33 bands
    # band edges: the 16 kHz octave reaches 22387 Hz, the 20 kHz third-octave 22387 Hz
    assert status(1000, 48000, 1, -5, 4) == L_.DSP_OK and status(1000, 44100, 1, -5, 4) == L_.DSP_ERR_INVALID
    assert status(1000, 48000, 3, -16, 13) == L_.DSP_OK and status(1000, 44100, 3, -16, 13) == L_.DSP_ERR_INVALID
    assert status(1000, 44100, 3, -16, 12) == L_.DSP_OK and status(1000, 48000, 3, -16, 14) == L_.DSP_ERR_INVALID
    assert status(1 << 24, 48000, 1, 0, 0) == L_.DSP_ERR_UNSUPPORTED  # L + P > 2^24


@pytest.mark.parametrize("bands", [(1, -5, 4), (3, -16, 13), (1, 3, 3)])
def test_plan_values(bands):
    sr = 48000
    m = dm.plan(1, sr, *bands)
    for k in (17, 18):
        at, past = d.decay_plan((1 << k) - m["P"], sr, *bands), d.decay_plan((1 << k) - m["P"] + 1, sr, *bands)
        assert at["n"] == 1 << k and past["n"] == 2 << k and at["P"] == past["P"] == m["P"]
    p = d.decay_plan(5, sr, *bands)
    assert p["n"] == max(1024, 1 << (5 + m["P"] - 1).bit_length()) and p["bands"] == m["bands"]
    assert np.allclose(p["fm"], m["fm"], rtol=1e-14, atol=0)
    assert p["P"] == math.ceil(8 * sr * m["Qr"] / m["fm"][0])


def test_scratch_is_capped():
    """The rows of a group hold at most 256 MiB, one row at least: 320 MiB + words at n = 2^24."""
    for L in (1000, 1 << 16, 1 << 20, (1 << 24) - (1 << 20)):
        p = d.decay_plan(L, 48000, 1, -5, 4, 64)
        row = 8 * p["n"] + 2 * (4 * p["n"] + 8) + 4 * ((L + 1) & ~1)
        rows = min(16, max(1, (256 << 20) // row))
        assert p["scratch_bytes"] == rows * (row + 16 * p["hops"])
        assert p["scratch_bytes"] <= max(256 << 20, row) + rows * 16 * p["hops"]


def test_result_layout():
    assert C.sizeof(L_.dsp_decay_result) == 80
    assert [getattr(L_.dsp_decay_result, f).offset for f in FIELDS] == [8 * i for i in range(8)]
    assert L_.dsp_decay_result.flags.offset == 64 and L_.dsp_decay_result.truncation.offset == 68
    assert C.sizeof(L_.dsp_decay_spec) == 12


def close(got, want, rel=1e-9):
    for k in FIELDS:
        g, w = got[k], want[k]
        assert (math.isnan(g) and math.isnan(w)) or g == w or abs(g - w) <= rel * abs(w), (k, g, w)
    assert got["flags"] == want["flags"] and got["truncation"] == want["truncation"]


def noisy_ir(sr, seconds, T, noise_db, seed, lead=20):
    rng = np.random.default_rng(seed)
    L = int(seconds * sr)
    t = np.arange(L - lead) / sr
    h = np.zeros(L)
    h[lead:] = rng.standard_normal(L - lead) * np.exp(-6.9078 * t / T)
    h[lead] = 4.0
    h += 10.0 ** (noise_db / 20.0) * rng.standard_normal(L)
    return (0.2 * h).astype(np.float32)


@pytest.mark.parametrize("sr,noise_db", [(48000, -70.0), (44100, -30.0), (32000, -15.0)])
def test_derive_against_model(sr, noise_db):
    h = noisy_ir(sr, 0.8, 0.25, noise_db, 3)
    bands = (1, -2, 2)
    _, onset, e, m = dm.energies64(h[None, :], sr, *bands)
    hop = dm.hop_of(sr)
    for b in range(e.shape[1]):
        want = dm.derive(e[0, b], m[0, b], len(h), int(onset[0]), hop, sr)
        close(d.decay_derive(e[0, b], m[0, b], len(h), int(onset[0]), hop, sr), want)
        no_m = d.decay_derive(e[0, b], None, len(h), int(onset[0]), hop, sr)
        assert math.isnan(no_m["ts"]) and no_m["t20"] == pytest.approx(want["t20"], rel=1e-9, nan_ok=True)


def synthetic_row(sr, inr_db, T=0.4, seconds=1.2):
    """An energy row: a pure exponential plus a floor placed for the wanted INR."""
    hop = dm.hop_of(sr)
    L = int(seconds * sr)
    hops = -(-L // hop) + 1
    j = np.arange(hops - 1)
    decay = np.exp(-13.8155 * j * hop / sr / T)
    W = (sr // 100) // hop
    floor = decay[:W].mean() / (10.0 ** (inr_db / 10.0) - 1.0)
    e = np.concatenate([[0.0], decay + floor])
    return e, L, hop


@pytest.mark.parametrize("sr", [48000, 44100])
@pytest.mark.parametrize("thr,flag", [(20.0, dm.EDT_INVALID), (35.0, dm.T20_INVALID), (45.0, dm.T30_INVALID)])
def test_validity_flags_either_side_of_each_threshold(sr, thr, flag):
    for delta, valid in ((-0.05, False), (0.05, True)):
        e, L, hop = synthetic_row(sr, thr + delta)
        want = dm.derive(e, None, L, 0, hop, sr)
        assert (want["inr"] >= thr) == valid and abs(want["inr"] - thr) < 0.1
        got = d.decay_derive(e, None, L, 0, hop, sr)
        close(got, want)
        assert bool(got["flags"] & flag) == (not valid)
        name = {dm.EDT_INVALID: "edt", dm.T20_INVALID: "t20", dm.T30_INVALID: "t30"}[flag]
        assert math.isnan(got[name]) == (not valid)


def test_silent_row():
    sr, hop, L = 48000, 48, 4800
    e = np.zeros(-(-L // hop) + 1)
    got = d.decay_derive(e, e.copy(), L, 0, hop, sr)
    assert got["flags"] & L_.DSP_DECAY_SILENT and all(math.isnan(got[k]) for k in FIELDS)
    close(got, dm.derive(e, e, L, 0, hop, sr))


def test_row_shorter_than_10_ms():
    sr, hop = 48000, 48
    for L, short in ((479, True), (480, False)):
        e = np.concatenate([[0.0], np.exp(-0.5 * np.arange(-(-L // hop)))])
        got = d.decay_derive(e, None, L, 0, hop, sr)
        close(got, dm.derive(e, None, L, 0, hop, sr))
        assert bool(got["flags"] & L_.DSP_DECAY_SHORT) == short
        assert all(math.isnan(got[k]) for k in FIELDS) == short


def test_derive_refusals():
    res = L_.dsp_decay_result()
    e = np.ones(11)
    p = d.api._dptr(e)
    f = L_.lib().dsp_decay_derive
    assert f(p, None, 480, 0, 48, 48000, C.byref(res)) == L_.DSP_OK
    assert f(None, None, 480, 0, 48, 48000, C.byref(res)) == L_.DSP_ERR_INVALID
    assert f(p, None, 480, 0, 48, 48000, None) == L_.DSP_ERR_INVALID
    assert f(p, None, 480, 481, 48, 48000, C.byref(res)) == L_.DSP_ERR_INVALID
    assert f(p, None, 480, 0, 47, 48000, C.byref(res)) == L_.DSP_ERR_INVALID
    assert f(p, None, 480, 0, 21, 22050, C.byref(res)) == L_.DSP_ERR_INVALID


@pytest.mark.parametrize("sr", [48000, 44100])
def test_known_answer_through_the_float64_model(sr):
    """Decaying sines at the 126, 1000 and 7943 Hz octave mids with T = 1.0, 0.6, 0.3 s, 1.5 s
    long after 37 zeros: EDT, T20 and T30 within 0.2 % of the designed T; C50 = -0.18, 3.32
    and 9.54 dB (a pure exponential's 10 log10(e^(13.8 * 0.05 / T) - 1) is -0.02, 3.32 and
    9.54 dB: the 126 Hz sine's 6.3 periods in 50 ms do not average out).  The library's
    derive step on the same energies agrees with the model's to 1e-9."""
    h = dm.decaying_sines(sr)
    bands = (1, -3, 3)
    _, onset, e, m = dm.energies64(h[None, :], sr, *bands)
    assert int(onset[0]) == 38
    hop = dm.hop_of(sr)
    for b, T, c50 in ((0, 1.0, -0.18), (3, 0.6, 3.32), (6, 0.3, 9.54)):
        r = dm.derive(e[0, b], m[0, b], len(h), 38, hop, sr)
        assert r["flags"] == 0
        for k in ("edt", "t20", "t30"):
            assert abs(r[k] - T) <= 0.002 * T, (k, r[k], T)
        assert abs(r["c50"] - c50) <= 0.006, (r["c50"], c50)
        close(d.decay_derive(e[0, b], m[0, b], len(h), 38, hop, sr), r)
