"""dsp_limiter on the GPU (limiter.hip) against the float64 model of
tests/limiterutil.py and against itself: the ceiling, the identity, the detector
rows, the pinned division, the model, linking, prefixes, reproducibility and
row layouts.  Every case's device results and float64 model are computed once
(run_case) and shared."""
import ctypes
import functools

import numpy as np
import pytest

import dspbench as d
from dspbench import _lib as L
import limiterutil as lu
import rowsutil as ru
from test_gpu_resample import RESAMPLE_TOL

pytestmark = pytest.mark.gpu

C0 = lu.CEILING
IDS = [lu.case_id(k) for k in lu.CASES]


def spec_of(k, A=None, tau=None):
    flags = (L.DSP_LIMITER_TRUE_PEAK if k["true_peak"] else 0) | (0 if k["linked"] else L.DSP_LIMITER_UNLINKED)
    return L.dsp_limiter_spec(C0, k["A"] if A is None else A, float(k["tau"] if tau is None else tau), flags)


def call(torch, x, k, host=False, out=None, **kw):
    """(y, g, p, info) as numpy from one call on x [C, L] (numpy)."""
    xin = x if host else torch.from_numpy(np.array(x)).cuda()
    y, info = d.limiter(xin, k["sr"], spec=spec_of(k, **kw), return_gain=True, return_detector=True, out=out)
    back = (lambda t: t) if host else (lambda t: t.cpu().numpy())
    return back(y), back(info["gain"]), back(info["detector"]), info


@functools.lru_cache(None)
def run_case(i):
    import torch
    k = lu.CASES[i]
    x = lu.case_input(k)
    y, g, p, info = call(torch, x, k)
    g64, y64, p64 = lu.limiter64(x, k["sr"], C0, k["A"], k["tau"], k["true_peak"], k["linked"])
    for a in (x, y, g, p):
        a.setflags(write=False)
    return dict(k=k, x=x, y=y, g=g, p=p, info=info, g64=g64, y64=y64, p64=p64)


def rows_of(k, c):
    """The link group of channel c as a row index of gain / detector."""
    return 0 if k["linked"] else c


@pytest.mark.parametrize("i", range(len(lu.CASES)), ids=IDS)
def test_ceiling(torch_cuda, i):
    r = run_case(i)
    ru.assert_finite(r["y"], r["g"])
    assert float(np.max(np.abs(r["y"]))) <= np.float32(C0)
    # the result against the gain row (a peak in a row shorter than the window may leave g = 1 to the clamp)
    assert r["info"]["min_gain"] == float(r["g"].min())
    assert r["info"]["limited"] == int(np.count_nonzero(r["g"] < np.float32(1.0)))


@pytest.mark.parametrize("true_peak,sr", [(False, 48000), (True, 192000)])
@pytest.mark.parametrize("C,Lx,A,tau", [(1, 1, 0, 0), (2, 2049, 64, 4800), (17, 4166, 1024, 64), (3, 300, 63, 64)])
def test_identity(torch_cuda, C, Lx, A, tau, true_peak, sr):
    # (an oversampled detector overshoots a full-scale input; at ovs = 1 the flag changes nothing)
    x = lu.quiet(C + Lx, C, Lx, C0)
    for linked in (True, False):
        k = dict(A=A, tau=tau, sr=sr, true_peak=true_peak, linked=linked)
        y, g, p, info = call(torch_cuda, x, k)
        assert ru.same_bits(y, x)
        assert np.all(g == np.float32(1.0))
        assert info["limited"] == 0 and info["min_gain"] == 1.0


def test_empty_rows(torch_cuda):
    x = torch_cuda.zeros((2, 4), dtype=torch_cuda.float32, device="cuda")[:, :0]
    y, info = d.limiter(x, 48000)
    assert tuple(y.shape) == (2, 0) and info == {"min_gain": 1.0, "limited": 0}


@pytest.mark.parametrize("i", range(len(lu.CASES)), ids=IDS)
def test_detector_rows(torch_cuda, i):
    r = run_case(i)
    k = r["k"]
    if k["true_peak"] and lu.oversample(k["sr"]) > 1:
        # the oversampled detector: dsp_resample's sum, within its bound of the float64 rows; never below |x|
        assert np.max(np.abs(r["p"] - r["p64"])) <= RESAMPLE_TOL * np.max(r["p64"])
        groups = [list(range(k["C"]))] if k["linked"] else [[c] for c in range(k["C"])]
        for j, rows in enumerate(groups):
            assert np.all(r["p"][j] >= np.abs(r["x"][rows]).max(axis=0))
        return
    groups = [list(range(k["C"]))] if k["linked"] else [[c] for c in range(k["C"])]
    for j, rows in enumerate(groups):
        assert ru.same_bits(r["p"][j], np.abs(r["x"][rows]).max(axis=0))


@pytest.mark.parametrize("sr", [48000, 96000])
def test_detector_true_peak_impulses(torch_cuda, sr):
    """Unit impulses more than Tp apart: every oversampled output has one
    non-zero product, so p is |amp x a table entry| maxed over the phases of
    each input sample -- and |amp| itself at the impulse -- bit for bit."""
    ovs = lu.oversample(sr)
    T = d.resample_taps(sr, sr * ovs)  # [ovs, Tp] float32
    Tp = T.shape[1]
    half = Tp // 2
    Lx = 2048 + 3 * Tp + 50
    at = [5, 5 + Tp + 7, 2040, 2040 + Tp + 40, Lx - 3]
    amps = np.array([0.5, -1.75, 3.0, -0.3, 2.0], np.float32)
    x = np.zeros((1, Lx), np.float32)
    x[0, at] = amps
    want = np.abs(x[0]).copy()
    for n0, amp in zip(at, amps):
        for i in range(Tp):  # u[ovs n + phi] = table[phi][i] x[n - half + 1 + i]: n = n0 + half - 1 - i
            n = n0 + half - 1 - i
            if 0 <= n < Lx:
                want[n] = max(want[n], np.max(np.abs(T[:, i] * amp)))
    k = dict(A=0, tau=0, sr=sr, true_peak=True, linked=True)
    _, _, p, _ = call(torch_cuda, x, k)
    assert ru.same_bits(p[0], want)


@pytest.mark.parametrize("sr", [48000, 96000])
def test_detector_is_the_meters_oversampler(torch_cuda, sr):
    """the limiter's true-peak detector is the meter's
    oversampler.  For one input the maximum of the linked detector row equals
    max(sample_peak, true_peak) of dsp_loudness bit for bit (limiter.hip's
    OVS > 1 branch and loudness.hip's loudness_truepeak_kernel sum the same
    products in the same order).  The rows cross a tile of both kernels and
    start one float off 16-byte alignment."""
    C, Lx = 2, 2048 + 1024 + 37
    base = torch_cuda.zeros((C, Lx + 3), dtype=torch_cuda.float32, device="cuda")  # rows 16-byte aligned
    x = base[:, 1:1 + Lx]
    x.copy_(torch_cuda.from_numpy(np.random.default_rng(sr).uniform(-1, 1, (C, Lx)).astype(np.float32)))
    assert all(x[c].data_ptr() % 16 == 4 for c in range(C))
    k = dict(A=0, tau=0, sr=sr, true_peak=True, linked=True)
    _, info = d.limiter(x, sr, spec=spec_of(k), return_detector=True)
    p = info["detector"].cpu().numpy()
    m = d.loudness(x, sr, true_peak=True)
    assert lu.oversample(sr) > 1 and p.shape == (1, Lx)
    assert m["true_peak"] > 0.0 and m["sample_peak"] == float(np.abs(x.cpu().numpy()).max())
    assert float(p.max()) == max(m["sample_peak"], m["true_peak"])


@pytest.mark.parametrize("i", [j for j, k in enumerate(lu.CASES) if k["L"] in (2049, 20000)],
                         ids=lambda j: IDS[j])
def test_division_pinned(torch_cuda, i):
    """A = 0, tau = 0: g is numpy's float32 1 - (1 - c / p) where p > c, else 1, bit for bit."""
    r = run_case(i)
    _, g, p, _ = call(torch_cuda, r["x"], r["k"], A=0, tau=0)
    c = np.float32(C0)
    with np.errstate(divide="ignore"):
        want = np.where(p > c, np.float32(1.0) - (np.float32(1.0) - c / p), np.float32(1.0)).astype(np.float32)
    assert ru.same_bits(g, want)


@pytest.mark.parametrize("i", range(len(lu.CASES)), ids=IDS)
def test_model(torch_cuda, i):
    r = run_case(i)
    k, x = r["k"], r["x"].astype(np.float64)
    err = float(np.max(np.abs(r["g"] - r["g64"])))
    print(f"{IDS[i]}: max |g - g64| = {err:.3e}")
    assert err <= lu.LIM_TOL
    for c in range(k["C"]):
        g64 = r["g64"][rows_of(k, c)]
        want = np.clip(x[c] * g64, -C0, C0)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(r["y"][c] - want) <= lu.LIM_TOL * np.abs(x[c]) + ulp)


@pytest.mark.parametrize("i", [j for j, k in enumerate(lu.CASES) if k["linked"] and k["C"] > 1], ids=lambda j: IDS[j])
def test_linked(torch_cuda, i):
    r = run_case(i)
    assert r["g"].shape[0] == 1
    c = np.float32(C0)
    assert ru.same_bits(r["y"], np.clip(r["x"] * r["g"][0][None, :], -c, c))


@pytest.mark.parametrize("C,Lx,A,true_peak", [(3, 4166, 63, False), (17, 2049, 64, False), (17, 2100, 1, True)])
def test_unlinked_is_per_channel(torch_cuda, C, Lx, A, true_peak):
    x = lu.inputs(C * Lx, C, Lx, C0, A)
    k = dict(A=A, tau=4800, sr=48000, true_peak=true_peak, linked=False)
    y, g, p, info = call(torch_cuda, x, k)
    assert g.shape == (C, Lx)
    limited = 0
    for c in range(C):
        y1, g1, p1, i1 = call(torch_cuda, x[c:c + 1], k)
        assert ru.same_bits(y[c], y1[0]) and ru.same_bits(g[c], g1[0]) and ru.same_bits(p[c], p1[0])
        limited += i1["limited"]
    assert info["limited"] == limited


@pytest.mark.parametrize("A,tau,true_peak,sr", [(0, 64, False, 48000), (64, 4800, False, 48000), (1024, 4800, False, 48000),
                                                (63, 4800, True, 48000), (1, 64, True, 96000)])
def test_prefix(torch_cuda, A, tau, true_peak, sr):
    """The tile grid is anchored at 0: limiting x[:, :M] gives the same g and y
    on [0, M - A - half) as limiting x."""
    M, Lx = 2 * 2048 + 7, 3 * 2048 + 100
    x = lu.inputs(A + tau, 2, Lx, C0, A)
    x[1, M - 3] = np.float32(5 * C0)  # (inside the prefix's last samples: seen by both)
    x[0, M + 10] = np.float32(-6 * C0)  # (past the prefix: it reaches back A + half samples)
    k = dict(A=A, tau=tau, sr=sr, true_peak=true_peak, linked=True)
    half = d.resample_plan(sr, sr * lu.oversample(sr))["taps"] // 2 if true_peak else 0
    y, g, _, _ = call(torch_cuda, x, k)
    yp, gp, _, _ = call(torch_cuda, x[:, :M], k)
    n = M - A - half
    assert ru.same_bits(g[:, :n], gp[:, :n]) and ru.same_bits(y[:, :n], yp[:, :n])


@pytest.mark.parametrize("i", [j for j, k in enumerate(lu.CASES) if k["L"] >= 2047][::3], ids=lambda j: IDS[j])
def test_reproducible_paths(torch_cuda, i):
    r = run_case(i)
    k, x = r["k"], r["x"]
    y, g, p, info = call(torch_cuda, x, k)  # again
    assert ru.same_bits(y, r["y"]) and ru.same_bits(g, r["g"]) and ru.same_bits(p, r["p"])
    assert info["min_gain"] == r["info"]["min_gain"] and info["limited"] == r["info"]["limited"]
    xin = torch_cuda.from_numpy(np.array(x)).cuda()  # in place
    yt, it = d.limiter(xin, k["sr"], spec=spec_of(k), out=xin)
    assert yt.data_ptr() == xin.data_ptr() and ru.same_bits(xin.cpu().numpy(), r["y"])
    assert it["min_gain"] == info["min_gain"] and it["limited"] == info["limited"]
    yh, gh, ph, ih = call(torch_cuda, np.array(x), k, host=True)  # host rows
    assert ru.same_bits(yh, r["y"]) and ru.same_bits(gh, r["g"]) and ru.same_bits(ph, r["p"])
    xh = np.array(x)
    d.limiter(xh, k["sr"], spec=spec_of(k), out=xh)  # host rows in place
    assert ru.same_bits(xh, r["y"])
    # the result against the gain row
    assert info["min_gain"] == float(r["g"].min())
    assert info["limited"] == int(np.count_nonzero(r["g"] < np.float32(1.0)))


def test_no_result_is_stream_ordered(torch_cuda):
    k = lu.CASES[IDS.index(next(s for s in IDS if s.startswith("A64-L20000")))]
    r = run_case(lu.CASES.index(k))
    xin = torch_cuda.from_numpy(np.array(r["x"])).cuda()
    y, info = d.limiter(xin, k["sr"], spec=spec_of(k), result=False)
    assert info == {}
    torch_cuda.cuda.synchronize()
    assert ru.same_bits(y.cpu().numpy(), r["y"])


def test_overlap_refused(torch_cuda):
    x = torch_cuda.zeros((3, 4096), dtype=torch_cuda.float32, device="cuda")
    with pytest.raises(L.DspError) as e:
        d.limiter(x[:2, :4000], 48000, out=x[:2, 8:4008])  # shifted by 8 samples: neither apart nor in place
    assert e.value.status == -1
    with pytest.raises(L.DspError) as e:  # out[0] is in[1]
        d.limiter(x[0:2], 48000, out=x[1:3])
    assert e.value.status == -1
    with pytest.raises(L.DspError) as e:  # the gain row is an input row
        L.check(L.lib().dsp_limiter(L.chan_table([x[0].data_ptr()]), 1, 4096, L.chan_table([x[1].data_ptr()]), 48000,
                                    ctypes.byref(spec_of(dict(A=1, tau=0, true_peak=False, linked=True))), None,
                                    L.chan_table([x[0].data_ptr()]), None, None,
                                    ctypes.byref(d.api._exec(x))), "dsp_limiter")
    assert e.value.status == -1


@pytest.mark.parametrize("layout", ru.ALL)
@pytest.mark.parametrize("true_peak,linked,Lx", [(False, True, 4166), (True, False, 2300), (True, True, 300)])
def test_rows(torch_cuda, layout, true_peak, linked, Lx):
    """Unaligned starts, strided rows, NaN-filled gaps and guards: nothing
    outside the rows is written, no sample outside [0, L) is consumed, and the
    results are the aligned call's."""
    C, A = 3, 64
    x = lu.inputs(Lx + C, C, Lx, C0, A)
    k = dict(A=A, tau=4800, sr=48000, true_peak=true_peak, linked=linked)
    base = base_rows(true_peak, linked, Lx)
    oi, oo, sm = ru.LAYOUTS[layout]
    G = 1 if linked else C
    for host in (False, True):
        t = None if host else torch_cuda
        xin = ru.Rows(C, Lx + 5, oi, sm, t).fill(x, Lx)
        out, gain, det = ru.Rows(C, Lx, oo, sm, t), ru.Rows(G, Lx, oo, sm, t), ru.Rows(G, Lx, oi, sm, t)
        sp = spec_of(k)
        ex = d.api._exec(xin.view if not host else None, 0, None)
        res = L.dsp_limiter_result()
        L.check(L.lib().dsp_limiter(L.chan_table(xin.ptrs()), C, Lx, L.chan_table(out.ptrs()), 48000, ctypes.byref(sp),
                                    None, L.chan_table(gain.ptrs()), L.chan_table(det.ptrs()), ctypes.byref(res),
                                    ctypes.byref(ex)), "dsp_limiter")
        for r in (out, gain, det):
            r.check_output()
        got = (out.numpy(), gain.numpy(), det.numpy())
        ru.assert_finite(*got)
        for a, b in zip(got, base[:3]):
            assert ru.same_bits(a, b)
        assert (res.min_gain, res.limited) == base[3]
        assert np.all(xin.numpy(Lx).view(np.int32) == x.view(np.int32))  # the input rows are left alone


@functools.lru_cache(None)
def base_rows(true_peak, linked, Lx):
    import torch
    C, A = 3, 64
    x = lu.inputs(Lx + C, C, Lx, C0, A)
    y, g, p, info = call(torch, x, dict(A=A, tau=4800, sr=48000, true_peak=true_peak, linked=linked))
    return y, g, p, (info["min_gain"], info["limited"])
