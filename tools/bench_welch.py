#!/usr/bin/env python3
"""dsp_welch on one hour of 48 kHz stereo, with and without a reference row:
HIP events around the call, median of 5 after one warm-up.  Beside it
dsp_stft_magnitude of the same hour (what a host-side average had to start
from) and scipy.signal.welch on one CPU thread (on --scipy-seconds of the
signal, scaled to the hour; scipy.fft runs one worker unless told otherwise,
and the thread-count variables are set before anything is imported).  One JSON
line per measurement; the output file is written anew on every run.

The algorithmic bytes of dsp_welch are one read of the rows (1.38 GB, 2.07 GB
with the reference); the fraction of the 8 TB/s roof is reported against them.
What the launches move beyond that -- every frame's spectrum written to the
scratch and read back, 33792 bytes a frame and row against 16384 bytes of
samples at hop 4096 -- is reported as scratch_bytes.
"""
import os
os.environ["OMP_NUM_THREADS"] = os.environ["MKL_NUM_THREADS"] = os.environ["OPENBLAS_NUM_THREADS"] = "1"  # before numpy
import argparse  # noqa: E402
import json  # noqa: E402
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dsp-bench_amd"))
ROOF = 8.0e12


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--hop", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-seconds", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "welch_bench.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import dspbench as d

    sr, C = 48000, a.channels
    L = int(a.seconds * sr)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((C, L), generator=g, device="cuda", dtype=torch.float32) * 0.25
    ref = torch.randn((L,), generator=g, device="cuda", dtype=torch.float32) * 0.25
    lines = []
    for has_ref in (False, True):
        p = d.welch_plan(L, C, has_ref, a.hop)
        med, ms = timed(torch, lambda: d.welch_sums(x, ref if has_ref else None, a.hop), a.reps)
        rows = C + (1 if has_ref else 0)
        algo = 4 * L * rows
        lines.append({"what": "dsp_welch", "seconds": a.seconds, "channels": C, "ref": has_ref, "hop": a.hop,
                      "frames": p["frames"], "median_ms": med, "all_ms": ms, "algorithmic_bytes": algo,
                      "algorithmic_GBps": algo / med / 1e6, "fraction_of_roof": algo / (med * 1e-3) / ROOF,
                      "scratch_bytes": 2 * 33792 * p["frames"] * rows, "plan_scratch_bytes": p["scratch_bytes"]})
    mag = torch.empty((C, d.stft_frames(L, 8192, a.hop), 4097), device="cuda", dtype=torch.float32)
    med, ms = timed(torch, lambda: d.stft_magnitude(x, 8192, a.hop, d.DSP_WIN_HANN, out=mag), a.reps)
    lines.append({"what": "dsp_stft_magnitude", "seconds": a.seconds, "channels": C, "hop": a.hop, "median_ms": med,
                  "all_ms": ms, "bytes_written": mag.numel() * 4})
    del mag
    try:
        from scipy import signal
        torch.set_num_threads(1)
        n = min(L, int(a.scipy_seconds * sr))
        xs = x[:, :n].cpu().numpy().astype(np.float64)
        w = signal.get_window("hann", 8192, fftbins=False)
        t0 = time.perf_counter()
        signal.welch(xs, fs=sr, window=w, nperseg=8192, noverlap=8192 - a.hop, detrend=False)
        dt = time.perf_counter() - t0
        lines.append({"what": "scipy.signal.welch, one CPU thread", "measured_seconds_of_signal": n / sr,
                      "measured_ms": dt * 1e3, "scaled_to_ms": dt * 1e3 * L / n, "channels": C, "hop": a.hop})
    except ImportError:
        lines.append({"what": "scipy.signal.welch", "skipped": "scipy is not installed"})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            f.write(s + "\n")


if __name__ == "__main__":
    main()
