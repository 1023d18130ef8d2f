"""The older STFT / FFT kernels on inputs whose spectra are known in closed
form (stftutil.py): one frame is one case.

Every other STFT test feeds white noise, where each sample, window value and
twiddle is about 1/sqrt(N) of every bin and a defect confined to one index
passes the peak-relative bar (test_stft_closed_forms_cpu.py counts it).  Here

  * a single impulse at j makes every bin |amp| w[j] / sqrt(N): one window
    sample, one input lane, seen alone;
  * two impulses interfere, |a1 w[j1] + a2 w[j2] exp(-2 i pi k (j2 - j1) / N)|:
    magnitudes see twiddle phase and the partner selection of the real split;
  * a bin-centred tone puts the frame into one output bin.

Paths: the packed 8192-point kernel with the computed window (K = 4097), the
table window (K = 4096, 1000) and the mirror (K = 8192); the generic LDS FFT
at N = 8192 (a row offset by one float, and H = 8193) and at every N = 4 ..
4096; overlapping frames (H = 4096, 2048) at F = 1, 5, 67; the fused render +
STFT with no_op and gain_test; fft_forward / fft_reverse at n = 2 .. 8192,
where re and im (phase) are checked directly.

Bars are stftutil's: check_frames (the project's per-frame peak-relative 1e-6
+ 2^-61) for tones, the same 1e-6 of the largest magnitude the amplitudes can
produce for impulses and pairs, and test_fft_services' 4e-6 of the peak for
re / im.  Every test prints `closed-forms-worst <case> <figure>`: its worst
error in units of its bar (measured: profiles/stft_closed_forms.txt).
"""
import functools

import numpy as np
import pytest

import dspbench as d
import oracle as orc
import stftutil as su
from test_gpu_parity import PEAK_REL_TOL

pytestmark = pytest.mark.gpu

N8 = 8192
SR = 48000.0
WINDOWS = {"hann": d.DSP_WIN_HANN, "hamming": d.DSP_WIN_HAMMING, "rect": d.DSP_WIN_RECT}
AMPS = (1.0, -0.75)                       # impulses: row 0, row 1
PAIR_AMPS = ((1.0, -0.625), (0.5, 0.75))  # pairs: (a1, a2) of row 0, row 1
TONES = ((0.5, 0.3), (0.25, 1.9))         # tones: (amp, phase) of row 0, row 1
FFT_TOL = 4e-6                            # test_gpu_parity.test_fft_services: 1e-6 * peak * 4, re and im apart


def record(request, worst):
    print(f"closed-forms-worst {request.node.name} {worst:.3f}")


def dev(torch, x):
    return torch.from_numpy(np.array(x, np.float32)).cuda()        # (a copy: the cached signals are read-only)


def test_bars_are_the_projects(torch_cuda):
    import test_gpu_edge_values as tev
    assert su.PEAK_REL_TOL == PEAK_REL_TOL and su.ABS_FLOOR == tev.ABS_FLOOR
    assert (orc.WIN_HANN, orc.WIN_HAMMING, orc.WIN_RECT) == (d.DSP_WIN_HANN, d.DSP_WIN_HAMMING, d.DSP_WIN_RECT)


# ---------------------------------------------------------------------------
# families: two rows per call, each row its own amplitudes
# ---------------------------------------------------------------------------
@functools.lru_cache(None)
def cases(N, family):
    return {"impulses": su.impulse_positions, "pairs": su.impulse_pairs, "tones": su.tone_bins}[family](N)


@functools.lru_cache(None)
def signal(N, family, hop=None):
    """[2, L] float32 (read-only)"""
    c = cases(N, family)
    if family == "impulses":
        x = np.stack([su.impulse_frames(N, c, a, hop) for a in AMPS])
    elif family == "pairs":
        x = np.stack([su.pair_frames(N, c, a1, a2, hop) for a1, a2 in PAIR_AMPS])
    else:
        x = np.stack([su.tone_frames(N, c, a, ph, hop) for a, ph in TONES])
    x.setflags(write=False)
    return x


@functools.lru_cache(None)
def tone_reference(N, window, row, full):
    """float64 magnitudes of the tone row, [F, N/2 + 1] or all N bins (read-only)"""
    ref = su.tone_mag(N, N if full else N // 2 + 1, window, signal(N, "tones")[row])
    ref.setflags(write=False)
    return ref


def check_family(mag, N, family, window, what, gain=1.0):
    """mag [2, F, K] of signal(N, family) times gain; the worst row's figure"""
    c, K = cases(N, family), mag.shape[2]
    assert mag.shape[:2] == (2, len(c)), mag.shape
    worst = 0.0
    for row in range(2):
        w = f"{what} row {row}"
        if family == "impulses":
            r = su.check_impulses(mag[row], N, c, AMPS[row] * gain, window, w)
        elif family == "pairs":
            a1, a2 = PAIR_AMPS[row]
            r = su.check_pairs(mag[row], N, c, a1 * gain, a2 * gain, window, w)
        else:
            ref = tone_reference(N, window, row, K > N // 2 + 1) * gain
            r = su.check_tones(mag[row], ref[:, :K], c, w, peak=ref.max(axis=1))    # (K = 1000: the peak may lie past it)
        worst = max(worst, r)
    return worst


# ---------------------------------------------------------------------------
# 8192-point memory-source STFT
# ---------------------------------------------------------------------------
PATHS = {
    # name: (K, H, rows offset by one float)
    "pk_computed_window": (4097, 8192, False),
    "pk_table_window_4096": (4096, 8192, False),
    "pk_table_window_1000": (1000, 8192, False),
    "pk_mirror": (8192, 8192, False),
    "generic_offset_rows": (4097, 8192, True),
    "generic_hop_8193": (4097, 8193, False),
}


def stft8k(torch, family, window, K, H, offset):
    x = signal(N8, family, None if H == N8 else H)
    L = x.shape[1]
    if offset:
        base = torch.zeros((2, L + 2), device="cuda")
        xin = base[:, 1:L + 1]
        xin.copy_(dev(torch, x))
        assert all(xin[c].data_ptr() % 8 == 4 for c in range(2))      # no row serves the packed kernel
    else:
        xin = dev(torch, x)
        assert H != N8 or all(xin[c].data_ptr() % 16 == 0 for c in range(2))
    mag = d.stft_magnitude(xin, N=N8, H=H, window=window, K=K).cpu().numpy()
    assert mag.shape == (2, len(cases(N8, family)), K)
    return mag


@pytest.mark.parametrize("wname", list(WINDOWS))
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("family", ["impulses", "pairs", "tones"])
def test_stft_8192(torch_cuda, request, family, path, wname):
    K, H, offset = PATHS[path]
    window = WINDOWS[wname]
    mag = stft8k(torch_cuda, family, window, K, H, offset)
    if K == N8:      # the mirror stores what the first half holds
        assert np.array_equal(mag[:, :, 1:4096].view(np.uint32), mag[:, :, :4096:-1].view(np.uint32))
    record(request, check_family(mag, N8, family, window, f"{family} {path} {wname}"))


@pytest.mark.parametrize("wname", list(WINDOWS))
@pytest.mark.parametrize("family", ["impulses", "pairs", "tones"])
def test_stft_8192_window_sources_agree(torch_cuda, request, family, wname):
    """K = 4097 computes its window, K = 1000 reads the table: the first 1000
    bins of the same input within 2 PEAK_REL_TOL of the frame peak (tones), or
    of the largest magnitude the amplitudes can produce (impulses, pairs: a
    frame's own peak is 1e-7 of that near a Hann window's ends, or zero)."""
    window = WINDOWS[wname]
    a = stft8k(torch_cuda, family, window, 4097, 8192, False).astype(np.float64)
    b = stft8k(torch_cuda, family, window, 1000, 8192, False).astype(np.float64)
    worst = 0.0
    for row in range(2):
        if family == "tones":
            scale = tone_reference(N8, window, row, False).max(axis=1)
        else:
            amps = [[AMPS[row]]] if family == "impulses" else [list(PAIR_AMPS[row])]
            scale = np.full(a.shape[1], su.sparse_scale(N8, window, amps)[0])
        ratio = np.abs(a[row, :, :1000] - b[row]).max(axis=1) / (2 * PEAK_REL_TOL * scale + su.ABS_FLOOR)
        f = int(np.argmax(ratio))
        msg = f"{family} {wname} row {row}: worst {ratio[f]:.3f} of the bar at frame {f} (case {cases(N8, family)[f]})"
        print(msg)
        assert ratio[f] <= 1.0, msg
        worst = max(worst, float(ratio[f]))
    record(request, worst)


# ---------------------------------------------------------------------------
# overlapping frames
# ---------------------------------------------------------------------------
SEG_OFFSETS = (0, 1, 127, 128, 129, 2047, 1000, 63, 64, 1777)


def overlap_signal(H, F, row):
    """one impulse in every hop of H samples: (x [L], J [F, N/H], A [F, N/H]),
    the in-frame positions and amplitudes of every frame's impulses"""
    L = N8 + (F - 1) * H
    seg = np.arange(L // H, dtype=np.int64)
    off = np.asarray(SEG_OFFSETS, np.int64)[(seg + 3 * row) % len(SEG_OFFSETS)]
    off = np.where(seg % 7 == 6, H - 1, off)                       # the last sample of a hop
    amp = np.where((seg + row) % 2 == 0, 1.0, -0.75)
    x = np.zeros(L, np.float32)
    x[seg * H + off] = amp
    M = N8 // H
    s = np.arange(F, dtype=np.int64)[:, None] + np.arange(M, dtype=np.int64)[None, :]
    return x, off[s] + np.arange(M, dtype=np.int64)[None, :] * H, amp[s]


@pytest.mark.parametrize("wname", ["hann", "rect"])
@pytest.mark.parametrize("F", [1, 5, 67])
@pytest.mark.parametrize("H", [4096, 2048])
def test_stft_8192_overlap(torch_cuda, request, H, F, wname):
    """Every impulse appears in N / H frames, at j, j - H, ...: each appearance
    matches the closed form for its in-frame position (frame addressing, and
    the workgroup remap at frame counts that are no multiple of 4 or 8)."""
    window = WINDOWS[wname]
    rows = [overlap_signal(H, F, row) for row in range(2)]
    mag = d.stft_magnitude(dev(torch_cuda, np.stack([r[0] for r in rows])), N=N8, H=H, window=window,
                           K=4097).cpu().numpy()
    assert mag.shape == (2, F, 4097)
    worst = 0.0
    for row, (_, J, A) in enumerate(rows):
        assert J.shape == (F, N8 // H) and J.min() >= 0 and J.max() < N8
        names = [f"frame {f}: j={J[f].tolist()}" for f in range(F)]
        worst = max(worst, su.check_sparse(mag[row], N8, J, A, window, names, f"overlap H={H} F={F} row {row}"))
    record(request, worst)


# ---------------------------------------------------------------------------
# fused render + STFT
# ---------------------------------------------------------------------------
FUSED_PLUGINS = {"no_op": (lambda: d.Plugin.no_op(), 1.0), "gain_test": (lambda: d.Plugin.gain_test(0.5), 0.5)}


def fused(torch, x, C_out, B, pname):
    """render bit-exact against x * gain (zeros past the file), then the magnitudes [C_out, F, 4097]"""
    mk, gain = FUSED_PLUGINS[pname]
    L = x.shape[1]
    out, mag = d.render_stft(dev(torch, x), C_out, B, SR, mk(), N=N8, H=N8, window=d.DSP_WIN_HANN, K=4097)
    out, mag = out.cpu().numpy(), mag.cpu().numpy()
    assert out.shape == (C_out, d.num_blocks(L, B) * B) and mag.shape == (C_out, L // N8, 4097)
    want = x * np.float32(gain)                                   # exact: a power of two
    assert np.array_equal(out[:, :L].view(np.uint32), want.view(np.uint32)) and not out[:, L:].any()
    return mag, gain


@pytest.mark.parametrize("family", ["impulses", "pairs"])
@pytest.mark.parametrize("B", [512, 384])
@pytest.mark.parametrize("pname", list(FUSED_PLUGINS))
def test_render_stft_fused(torch_cuda, request, pname, B, family):
    mag, gain = fused(torch_cuda, signal(N8, family), 2, B, pname)
    record(request, check_family(mag, N8, family, d.DSP_WIN_HANN, f"fused {pname} B={B} {family}", gain))


def test_render_stft_fused_three_channels(torch_cuda, request):
    """a channel group of odd size: impulses at 1.0 and -0.75, and the pairs' first row"""
    pos, pairs = cases(N8, "impulses"), cases(N8, "pairs")
    F = len(pos)
    x = np.zeros((3, F * N8), np.float32)
    x[:2] = signal(N8, "impulses")
    x[2, :len(pairs) * N8] = signal(N8, "pairs")[0]
    mag, gain = fused(torch_cuda, x, 3, 512, "gain_test")
    worst = max(su.check_impulses(mag[row], N8, pos, AMPS[row] * gain, d.DSP_WIN_HANN, f"fused C=3 row {row}")
                for row in range(2))
    a1, a2 = PAIR_AMPS[0]
    worst = max(worst, su.check_pairs(mag[2, :len(pairs)], N8, pairs, a1 * gain, a2 * gain, d.DSP_WIN_HANN,
                                      "fused C=3 row 2"))
    assert not mag[2, len(pairs):].any()                          # silence past the last pair
    record(request, worst)


# ---------------------------------------------------------------------------
# generic sizes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("wname", ["hann", "rect"])
@pytest.mark.parametrize("N", [1 << p for p in range(2, 13)])
def test_stft_generic_sizes(torch_cuda, request, N, wname):
    """the LDS FFT at every N = 4 .. 4096: every impulse position for N <= 1024
    (the seam set above), pairs and tones, H = N, K = N / 2 + 1, two rows"""
    window = WINDOWS[wname]
    worst = 0.0
    for family in ("impulses", "pairs", "tones"):
        x = signal(N, family)
        assert N > 1024 or x.shape[1] <= 1 << 20
        mag = d.stft_magnitude(dev(torch_cuda, x), N=N, H=N, window=window, K=N // 2 + 1).cpu().numpy()
        worst = max(worst, check_family(mag, N, family, window, f"N={N} {family} {wname}"))
    if N <= 1024:
        assert len(cases(N, "impulses")) == N
    record(request, worst)


# ---------------------------------------------------------------------------
# fft_forward / fft_reverse: re and im, so twiddle phase directly
# ---------------------------------------------------------------------------
def worst_of(got, ref, peak, names, what):
    """per case max|got - ref| in units of FFT_TOL * peak; got, ref [cases, n] (real), peak [cases]"""
    ratio = np.abs(got - ref).max(axis=1) / (FFT_TOL * peak)
    i = int(np.argmax(ratio))
    msg = f"{what}: worst {ratio[i]:.3f} of the bar at case {names[i]} (max err {np.abs(got - ref)[i].max():.3e}, peak {peak[i]:.3e})"
    print(msg)
    assert np.isfinite(got).all() and ratio[i] <= 1.0, msg
    return float(ratio[i])


def forward_all(torch, x):
    """fft_forward of every row of x [cases, n] -> float64 (re, im)"""
    xd = dev(torch, x)
    res = [d.fft_forward(xd[i]) for i in range(x.shape[0])]
    re = torch.stack([r[0] for r in res]).cpu().numpy().astype(np.float64)
    im = torch.stack([r[1] for r in res]).cpu().numpy().astype(np.float64)
    return re, im


@pytest.mark.parametrize("n", [1 << p for p in range(1, 14)])
def test_fft_services_closed_forms(torch_cuda, request, n):
    torch = torch_cuda
    m = np.arange(n, dtype=np.int64)
    tab = np.exp(-2j * np.pi * m / n)
    # an impulse at j: exp(-2 i pi j k / n) / sqrt(n); every j for n <= 1024, the seam set above
    pos = su.impulse_positions(n)
    re, im = forward_all(torch, su.impulse_frames(n, pos, 1.0).reshape(-1, n))
    ref = tab[(pos[:, None] * m[None, :]) % n] / np.sqrt(n)
    names, peak = [f"impulse j={j}" for j in pos], np.full(pos.size, 1 / np.sqrt(n))
    worst = max(worst_of(re, ref.real, peak, names, f"n={n} forward impulse re"),
                worst_of(im, ref.imag, peak, names, f"n={n} forward impulse im"))
    # bin-centred tones against float64 of the float32 signal
    bins = su.tone_bins(n)
    x = su.tone_frames(n, bins).reshape(-1, n)
    re, im = forward_all(torch, x)
    ref = np.fft.fft(x.astype(np.float64), axis=1) / np.sqrt(n)
    names, peak = [f"tone k={k}" for k in bins], np.abs(ref).max(axis=1)     # the spectrum's peak, as test_fft_services
    worst = max(worst, worst_of(re, ref.real, peak, names, f"n={n} forward tone re"),
                worst_of(im, ref.imag, peak, names, f"n={n} forward tone im"))
    # fft_reverse of a unit spectrum at k and its conjugate at n - k: 2 cos(2 pi k m / n) / sqrt(n)
    spec = np.zeros((bins.size, n), np.float32)
    spec[np.arange(bins.size), bins] = 1.0
    spec[np.arange(bins.size), (n - bins) % n] = 1.0
    sre, sim = dev(torch, spec), torch.zeros((bins.size, n), device="cuda")
    back = torch.stack([d.fft_reverse(sre[i], sim[i]) for i in range(bins.size)]).cpu().numpy().astype(np.float64)
    twice = np.where((bins == 0) | (2 * bins == n), 1.0, 2.0)[:, None]
    ref = twice * np.cos(2 * np.pi * ((bins[:, None] * m[None, :]) % n) / n) / np.sqrt(n)
    worst = max(worst, worst_of(back, ref, twice[:, 0] / np.sqrt(n), [f"reverse k={k}" for k in bins], f"n={n} reverse"))
    record(request, worst)
