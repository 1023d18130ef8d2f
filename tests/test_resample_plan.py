"""dsp_resample on the host: dsp_resample_plan, dsp_resample_taps (the table
the device uses) against the float64 model (resampleutil), the refusals, the
header's list of refused standard pairs, the ctypes layout of the spec."""
import ctypes as C
import itertools

import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L
import resampleutil as ru

PAIRS = [(44100, 48000), (48000, 44100), (48000, 96000), (96000, 48000), (44100, 96000), (48000, 2000),
         (48000, 48000)]
STANDARD = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000]
# include/dspbench/dspbench.h: the standard pairs refused at the default quality
REFUSED = set()


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
@pytest.mark.parametrize("Lx", [0, 1, 147, 5000])
def test_plan_matches_the_definition(sr_in, sr_out, Lx):
    got = d.resample_plan(sr_in, sr_out, Lx)
    want = ru.plan(sr_in, sr_out, Lx)
    assert (got["up"], got["down"], got["taps"], got["Lout"]) == (want["up"], want["down"], want["taps"], want["Lout"])
    assert got["table_bytes"] == 4 * want["up"] * want["taps"]
    assert got["Lout"] == -(-Lx * want["up"] // want["down"])


def test_plan_known_values():
    assert d.resample_plan(44100, 48000, 147) == {"up": 160, "down": 147, "taps": 136, "Lout": 160,
                                                  "table_bytes": 160 * 136 * 4}
    p = d.resample_plan(48000, 44100, 5000)
    assert (p["up"], p["down"], p["taps"], p["Lout"]) == (147, 160, 2 * 74, 4594)
    assert d.resample_plan(48000, 2000, 5000, zeros=4)["taps"] == 2 * int(np.ceil(4 * 24 / ru.DEFAULTS["rolloff"]))


def test_plan_accepts_null_outputs_and_null_spec():
    assert L.lib().dsp_resample_plan(44100, 48000, 10, None, None, None, None, None, None) == L.DSP_OK


@pytest.mark.parametrize("kw", [dict(sr_in=0), dict(sr_out=0), dict(zeros=3), dict(zeros=65), dict(beta=-0.1),
                                dict(beta=20.5), dict(beta=float("nan")), dict(rolloff=0.49), dict(rolloff=1.01)])
def test_plan_invalid(kw):
    a = dict(sr_in=44100, sr_out=48000, L_=100)
    a.update(kw)
    with pytest.raises(d.DspError) as e:
        d.resample_plan(**a)
    assert e.value.status == L.DSP_ERR_INVALID


@pytest.mark.parametrize("sr_in,sr_out,Lx", [
    (4099, 4097, 10),              # up = 4097 > 4096
    (192000, 1000, 10),            # taps = 2 ceil(64 * 192 / rolloff) = 25936 > 8192
    (16385, 4096, 10),             # up = 4096, taps = 542: a table of 8.9 MB > 8 MiB
    (44100, 48000, 1 << 62),       # L up overflows 2^63
])
def test_plan_unsupported(sr_in, sr_out, Lx):
    with pytest.raises(d.DspError) as e:
        d.resample_plan(sr_in, sr_out, Lx)
    assert e.value.status == L.DSP_ERR_UNSUPPORTED


def test_plan_limits_are_inclusive():
    assert d.resample_plan(4097, 4096, 10)["up"] == 4096                      # up = 4096 plans
    assert d.resample_plan(4001, 4096, 10)["table_bytes"] == 4096 * 136 * 4   # 2.2 MB
    assert d.resample_plan(44100, 48000, ((1 << 63) - 147) // 160)["Lout"] > 0


def test_standard_pairs_plan_or_are_listed():
    refused = set()
    for a, b in itertools.permutations(STANDARD, 2):
        st = L.lib().dsp_resample_plan(a, b, 48000, None, None, None, None, None, None)
        assert st in (L.DSP_OK, L.DSP_ERR_UNSUPPORTED), (a, b, st)
        if st != L.DSP_OK:
            refused.add((a, b))
    assert refused == REFUSED


@pytest.mark.parametrize("sr_in,sr_out,zeros", [(44100, 48000, 64), (48000, 44100, 16), (48000, 96000, 64),
                                                (96000, 48000, 4), (48000, 2000, 64), (44100, 96000, 16),
                                                (48000, 48000, 64)])
def test_taps_are_the_model_rounded(sr_in, sr_out, zeros):
    t = d.resample_taps(sr_in, sr_out, zeros=zeros)
    p = ru.plan(sr_in, sr_out, zeros=zeros)
    assert t.shape == (p["up"], p["taps"]) and t.dtype == np.float32
    want = ru.table64(p).astype(np.float32)
    # within 1 ulp of the model's float32 (two float64 evaluations of sin and I0 may round apart)
    ulp = np.spacing(np.maximum(np.abs(want), np.float32(1e-30)))
    assert np.all(np.abs(t.astype(np.float64) - want.astype(np.float64)) <= ulp)
    # the window's support: u = half - 1 - i + phi / up; zero exactly where |u| >= W
    u = (p["half"] - 1.0 - np.arange(p["taps"]))[None, :] + np.arange(p["up"])[:, None] / p["up"]
    assert not t[np.abs(u) >= p["W"]].any()


def test_taps_count_is_checked():
    buf = np.zeros(10, np.float32)
    st = L.lib().dsp_resample_taps(44100, 48000, None, buf.ctypes.data_as(L.FP), 10)
    assert st == L.DSP_ERR_INVALID


@pytest.mark.parametrize("sr_in,sr_out,zeros", [(44100, 48000, 64), (48000, 96000, 64), (44100, 96000, 16),
                                                (16000, 48000, 4)])
def test_phase_rows_sum_to_one(sr_in, sr_out, zeros):
    """Up-sampling: every phase row is a unit-DC-gain interpolator up to the
    window's stop-band leakage.  MARGIN is measured from the float64 model's own
    rows at these cases: max |sum(row64) - 1| is 1.5e-8 (Z = 64), 6.6e-8 (Z = 16,
    44100 -> 96000) and 2.2e-4 (Z = 4, where the short Kaiser window's images
    leak); the float32 rounding of Tp <= 136 taps, each below 1, adds at most
    Tp * 2^-25 = 4.1e-6.  The bound is the model's own deviation for the case
    (computed here, printed) plus that."""
    p = ru.plan(sr_in, sr_out, zeros=zeros)
    rows64 = ru.table64(p).sum(axis=1)
    model_dev = float(np.max(np.abs(rows64 - 1.0)))
    print(f"{sr_in}->{sr_out} Z={zeros}: float64 rows deviate {model_dev:.3e}")
    MARGIN = model_dev + p["taps"] * 2.0 ** -25
    t = d.resample_taps(sr_in, sr_out, zeros=zeros).astype(np.float64)
    assert np.max(np.abs(t.sum(axis=1) - 1.0)) <= MARGIN


def test_spec_layout():
    s = L.dsp_resample_spec
    assert C.sizeof(s) == 24
    assert (s.zeros.offset, s.beta.offset, s.rolloff.offset) == (0, 8, 16)
    assert L.lib().dsp_abi_version() == 3


def test_exports():
    for name in ("resample", "resample_plan", "resample_taps"):
        assert name in d.__all__ and callable(getattr(d, name))
