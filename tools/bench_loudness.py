"""bench_loudness.py -- dsp_loudness over one hour of stereo at 48 kHz, through
the public Python face only, timed with HIP events.

  python tools/bench_loudness.py [--seconds 3600] [--out profiles/loudness_bench.jsonl]

One child process per step, each under its own time limit; a step that fails
or runs out of time ends the run (nothing more is started on the GPU).  Steps,
each with a warm-up (tables, scratch) and the median of --reps:
  loudness          the K-weighted meter alone (no true peak)
  loudness_tp       with the true peak at the default quality
  loudness_tp16     with the true peak at zeros = 16
  biquad2           the two-section DSP_PLUGIN_BIQUAD render of the same hour with the K-weighting
                    coefficients (reads and writes every sample: the yardstick; the project's own
                    figure for that kernel is `bench.py --workload biquad --sections 2`)
  resample48_192    dsp_resample 48 -> 192 kHz of the same hour (writes 4 x the input)
  cpu               the float64 model on one core, 10 s scaled to the hour
The events bracket the whole call: dsp_loudness's time includes its copy of
the hop energies to the host, its stream synchronisation and the host gating.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dsp-bench_amd"))

SR = 48000
STEPS = ["loudness", "loudness_tp", "loudness_tp16", "biquad2", "resample48_192", "cpu"]


def gpu_step(step: str, seconds: int, reps: int) -> dict:
    import numpy as np
    import torch
    import dspbench as d
    C, L = 2, SR * seconds
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((C, L), generator=g, device="cuda") * 2 - 1
    extra = {}
    if step.startswith("loudness"):
        kw = {"true_peak": step != "loudness"}
        if step == "loudness_tp16":
            kw["zeros"] = 16
        def fn():
            return d.loudness(x, SR, **kw)
        extra["audio_bytes"] = 4 * C * L
    elif step == "biquad2":
        plug = d.Plugin.biquad(d.k_weighting(SR))
        out = torch.empty((C, d.num_blocks(L, 512) * 512), device="cuda")
        def fn():
            return d.render_offline(x, C, 512, float(SR), plug, out=out)
        extra["audio_bytes"] = 8 * C * L
    else:
        p = d.resample_plan(SR, 4 * SR, L)
        out = torch.empty((C, p["Lout"]), device="cuda")
        def fn():
            return d.resample(x, SR, 4 * SR, out=out)
        extra["audio_bytes"] = 4 * C * (L + p["Lout"])
    r = fn()   # warm-up
    torch.cuda.synchronize()
    if step.startswith("loudness"):
        extra.update({k: r[k] for k in ("integrated", "sample_peak", "true_peak", "blocks")})
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"step": step, "sr": SR, "seconds": seconds, "channels": C, "ms": sorted(ms),
            "ms_median": float(np.median(ms)), **extra}


def cpu_step(seconds: int) -> dict:
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import loudness_model
    sec = min(seconds, 10)
    t0 = time.perf_counter()
    loudness_model.timing(sec)
    dt = (time.perf_counter() - t0) * 1e3
    return {"step": "cpu_f64_model", "seconds_measured": sec, "ms_measured": dt,
            "ms_scaled_to_call": dt * seconds / sec}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loudness_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=120, help="time limit of each step, seconds")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        r = cpu_step(a.seconds) if a.child == "cpu" else gpu_step(a.child, a.seconds, a.reps)
        print("RESULT " + json.dumps(r))
        return 0
    lines = []
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--seconds", str(a.seconds), "--reps", str(a.reps),
               "--child", step]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"step {step}: time limit of {a.limit} s; stopping", file=sys.stderr)
            break
        res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(f"step {step}: exit {p.returncode}; stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            break
        print(res[0], flush=True)
        lines.append(res[0])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("".join(ln + "\n" for ln in lines))
    return 0 if len(lines) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
