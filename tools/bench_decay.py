#!/usr/bin/env python3
"""dsp_decay on 64 impulse responses of 2^20 samples at 48 kHz, octave (10 bands)
and third-octave (30 bands), with the moment rows: HIP events around the call,
median of 5 after one warm-up.  One JSON line per measurement; the output file
is written anew on every run.

The algorithmic bytes are one read of the rows and one write of the energy and
moment rows; the fraction of the 8 TB/s roof is reported against them.  What
the launches move beyond that -- per (channel, band) row a band spectrum
written and read, the inverse transform's passes over n points and the band
response written and read -- is reported as transform_points, rows * n.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dsp-bench_amd"))
ROOF = 8.0e12
BANDS = {"octave": (1, -5, 4), "third": (3, -16, 13)}


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
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--length", type=int, default=1 << 20)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decay_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import dspbench as d

    C, L, sr = a.rows, a.length, a.rate
    g = torch.Generator(device="cuda").manual_seed(1)
    t = torch.arange(L, device="cuda", dtype=torch.float32) / sr
    x = torch.randn((C, L), generator=g, device="cuda", dtype=torch.float32) * 0.25 * torch.exp(-6.9 * t / 2.0)
    lines = []
    for name, spec in BANDS.items():
        p = d.decay_plan(L, sr, *spec, C)
        med, ms = timed(torch, lambda: d.decay_energies(x, sr, *spec), a.reps)
        rows = C * p["bands"]
        algo = 4 * L * C + 2 * 8 * rows * p["hops"]
        lines.append({"what": "dsp_decay", "bands": name, "rows": C, "length": L, "rate": sr, "band_rows": rows,
                      "n": p["n"], "hop": p["hop"], "hops": p["hops"], "median_ms": med, "all_ms": ms,
                      "ms_per_band_row": med / rows, "algorithmic_bytes": algo, "algorithmic_GBps": algo / med / 1e6,
                      "fraction_of_roof": algo / (med * 1e-3) / ROOF, "transform_points": rows * p["n"],
                      "plan_scratch_bytes": p["scratch_bytes"]})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            s = json.dumps(ln)
            print(s)
            f.write(s + "\n")


if __name__ == "__main__":
    main()
