"""bench_resample.py -- dsp_resample over one hour of stereo at the default
quality, through the public Python face only, timed with HIP events.

  python tools/bench_resample.py [--seconds 3600] [--out profiles/resample_bench.jsonl]

One child process per step, each under its own time limit; a step that fails
or runs out of time ends the run (nothing more is started on the GPU).  Steps:
44100->48000, 48000->44100, 48000->96000, 96000->48000, each with a warm-up
(the table), median of --reps; then the float64 model on one CPU core (10 s of
stereo 44100->48000 scaled to the hour).  One JSON line per step, with the
yardsticks computed from the plan: the algorithmic bytes (input read once,
output written once) and the FP32 work of 2 Tp flop per output.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dsp-bench_amd"))

PAIRS = [(44100, 48000), (48000, 44100), (48000, 96000), (96000, 48000)]


def gpu_step(sr_in: int, sr_out: int, seconds: int, reps: int) -> dict:
    import numpy as np
    import torch
    import dspbench as d
    C, L = 2, sr_in * seconds
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((C, L), generator=g, device="cuda") * 2 - 1
    p = d.resample_plan(sr_in, sr_out, L)
    out = torch.empty((C, p["Lout"]), device="cuda")
    d.resample(x, sr_in, sr_out, out=out)   # warm-up: the table
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d.resample(x, sr_in, sr_out, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"step": f"resample{sr_in}_{sr_out}", "sr_in": sr_in, "sr_out": sr_out, "seconds": seconds, "channels": C,
            "up": p["up"], "down": p["down"], "taps": p["taps"], "ms": sorted(ms), "ms_median": float(np.median(ms)),
            "audio_bytes": 4 * C * (L + p["Lout"]), "flop": 2 * p["taps"] * C * p["Lout"]}


def cpu_step(seconds: int) -> dict:
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import resampleutil as ru
    sec = min(seconds, 10)
    x = ru.inputs(0, 2, 44100 * sec)
    t0 = time.perf_counter()
    for c in range(2):
        ru.resample_f64(x[c], 44100, 48000)
    dt = (time.perf_counter() - t0) * 1e3
    return {"step": "cpu_f64_model44100_48000", "seconds_measured": sec, "ms_measured": dt,
            "ms_scaled_to_call": dt * seconds / sec, "threads": int(os.environ.get("OMP_NUM_THREADS", "1"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=180, help="time limit of each step, seconds")
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        r = cpu_step(a.seconds) if a.child[0] == "cpu" else gpu_step(int(a.child[0]), int(a.child[1]), a.seconds,
                                                                     a.reps)
        print("RESULT " + json.dumps(r))
        return 0
    steps = [(str(i), str(o)) for i, o in PAIRS] + [("cpu", "0")]
    lines = []
    for s0, s1 in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--seconds", str(a.seconds), "--reps", str(a.reps),
               "--child", s0, s1]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"step {s0} {s1}: time limit of {a.limit} s; stopping", file=sys.stderr)
            break
        res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(f"step {s0} {s1}: exit {p.returncode}; stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            break
        print(res[0], flush=True)
        lines.append(res[0])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("".join(ln + "\n" for ln in lines))
    return 0 if len(lines) == len(steps) else 1


if __name__ == "__main__":
    sys.exit(main())
