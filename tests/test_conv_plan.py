"""DSP_PLUGIN_CONV on the host: dsp_conv_plan (the sizes the render itself
uses), the Python face's Plugin.conv, and the float64 FFT convolution the GPU
tests compare against, pinned here to the oracle's direct float64 sum."""
import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L
from convutil import conv_f64, conv_inputs

SPEC_BYTES = (2048 + 64) * 16  # one spectrum: 2048 float4 of paired bins and the bin-2048 slice


@pytest.mark.parametrize("T,parts", [(1, 1), (4096, 1), (4097, 2), (8192, 2), (8193, 3), (1 << 20, 256)])
def test_partitions(T, parts):
    assert d.conv_plan(T, 48000, 512, 2)[0] == parts


@pytest.mark.parametrize("Lx,B", [(0, 512), (1, 1), (100, 100), (4096, 512), (4097, 1), (12289, 100),
                                  (70001, 512), (172_800_000, 512)])
def test_frames(Lx, B):
    Lr = -(-Lx // B) * B
    _, frames, scratch = d.conv_plan(5000, Lx, B, 1)
    assert frames == -(-Lr // 4096)
    assert scratch == 2 * frames * SPEC_BYTES


def test_scratch_is_one_channel_group():
    s = [d.conv_plan(5000, 70001, 512, C)[2] for C in range(1, 40)]
    assert all(b > a for a, b in zip(s[:15], s[1:16]))   # monotone up to the group of 16
    assert all(v == s[15] for v in s[15:])               # then flat: groups reuse the scratch
    assert s[15] == 16 * s[0]


@pytest.mark.parametrize("T,B", [(0, 512), ((1 << 20) + 1, 512), (5000, 0)])
def test_plan_refusals(T, B):
    with pytest.raises(d.DspError) as e:
        d.conv_plan(T, 1000, B, 2)
    assert e.value.status == L.DSP_ERR_INVALID


def test_plan_accepts_null_outputs():
    assert L.lib().dsp_conv_plan(5000, 1000, 512, 2, None, None, None) == L.DSP_OK


def test_plugin_conv_blob():
    taps = np.arange(5000, dtype=np.float64)
    p = d.Plugin.conv(taps)
    assert p.kind == L.DSP_PLUGIN_CONV == 6
    assert p.params == taps.astype(np.float32).tobytes() and p.state == b""
    assert L.lib().dsp_abi_version() == 3


def test_fft_convolution_helper_is_the_direct_sum(oracle):
    x, taps = conv_inputs(0, 1, 3000, 5000)
    for Ly in (3072, 9000):
        want = oracle.fir_f64(x[0], taps, Ly)
        got = conv_f64(x[0], taps, Ly)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
