#!/usr/bin/env python3
"""dsp_limiter on one hour of 48 kHz stereo, linked, A = 72, tau = 4800: HIP
events around the call (no result: stream-ordered), the median of 5 after one
warm-up, sample mode and TRUE_PEAK, each beside its yardstick.
Appends one JSON line per mode to profiles/limiter_bench.jsonl.

  tools/bench_limiter.py [--seconds 3600] [--out profiles/limiter_bench.jsonl]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dsp-bench_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "limiter_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import dspbench as d
    from dspbench import _lib as L
    sr, C = 48000, 2
    n = a.seconds * sr
    g = torch.Generator(device="cuda").manual_seed(7)
    # noise at 0.3 of the ceiling with one sample in 4800 at 2-8 x the ceiling: every tile limits
    x = (torch.rand((C, n), generator=g, device="cuda") * 2 - 1) * 0.3 * 0.89
    x[:, ::4800] *= 20.0
    y = torch.empty_like(x)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    hbm = 6.4e12
    for mode, flags, yard_ms, yard in (
            ("sample", 0, 1e3 * (2 * 4 * C * n + 4 * C * n + 2 * 4 * n) / hbm,
             "x read twice, y written, h written and read at 6.4 TB/s"),
            ("true_peak", L.DSP_LIMITER_TRUE_PEAK, 4.46 * a.seconds / 3600.0, "loudness_truepeak_kernel<4>, 4.46 ms an hour")):
        spec = L.dsp_limiter_spec(0.89, 72, 4800.0, flags)
        times = []
        for it in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            d.limiter(x, sr, spec=spec, out=y, result=False)
            e1.record()
            torch.cuda.synchronize()
            if it:
                times.append(e0.elapsed_time(e1))
        times.sort()
        _, info = d.limiter(x, sr, spec=spec, out=y)
        rec = {"mode": mode, "seconds": a.seconds, "channels": C, "lookahead": 72, "release": 4800, "ms_median": times[2],
               "ms_all": times, "yardstick_ms": yard_ms, "yardstick": yard, "ratio": times[2] / yard_ms,
               "min_gain": info["min_gain"], "limited": info["limited"]}
        print(json.dumps(rec))
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
