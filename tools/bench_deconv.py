#!/usr/bin/env python3
"""dsp_rfft and dsp_deconvolve on stereo rows at n = 2^20 and n = 2^24: HIP
events around the call, the median of 5 after one warm-up, beside the
algorithmic bytes, the fraction of the HBM roofline they amount to, and
torch.fft.rfft on the same rows as a yardstick.  Appends one JSON
line per (n, operation) to profiles/deconv_bench.jsonl.

Algorithmic bytes: a transform of one row reads and writes M = n / 2 complex of
8 bytes in each of its passes (passes x 2 x 8 x M); the real split reads and
writes 8 (M + 1) more; the division reads Y and S and writes H (3 x 8 (M + 1)).

  tools/bench_deconv.py [--out profiles/deconv_bench.jsonl]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dsp-bench_amd"))

HBM = 8.0e12  # bytes per second, the part's peak


def median_ms(torch, fn):
    times = []
    for it in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it:
            times.append(e0.elapsed_time(e1))
    times.sort()
    return times[2], times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "deconv_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import dspbench as d
    C = 2
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for n in (1 << 20, 1 << 24):
        M = n // 2
        passes = d.rfft_plan(n)["passes"]
        g = torch.Generator(device="cuda").manual_seed(n)
        x = torch.rand((C, n), generator=g, device="cuda") * 2 - 1
        ref = torch.rand((n,), generator=g, device="cuda") * 2 - 1
        spec = torch.empty((C, n + 2), device="cuda")
        ir = torch.empty((C, n), device="cuda")
        one = passes * 2 * 8 * M + 2 * 8 * (M + 1)  # one row's transform
        cases = (
            ("rfft", lambda: d.rfft(x, n, out=spec), C * one, lambda: torch.fft.rfft(x)),
            ("irfft", lambda: d.irfft(spec, n, out=ir), C * one, lambda: torch.fft.irfft(torch.view_as_complex(spec.view(C, M + 1, 2)), n)),
            ("deconvolve", lambda: d.deconvolve(x, ref, out=ir), (2 * C + 1) * one + C * 3 * 8 * (M + 1), None),
        )
        for name, fn, nbytes, yard in cases:
            ms, all_ms = median_ms(torch, fn)
            rec = {"op": name, "n": n, "channels": C, "passes": passes, "ms_median": ms, "ms_all": all_ms,
                   "algorithmic_bytes": nbytes, "roofline_ms": 1e3 * nbytes / HBM, "hbm_fraction": 1e3 * nbytes / HBM / ms}
            if yard is not None:
                try:
                    rec["torch_fft_ms"] = median_ms(torch, yard)[0]
                except RuntimeError as e:  # (where torch offers it)
                    rec["torch_fft_ms"] = None
                    rec["torch_fft_error"] = str(e)[:200]
            print(json.dumps(rec))
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
