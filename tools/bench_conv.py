"""bench_conv.py -- DSP_PLUGIN_CONV over one hour of 48 kHz stereo, through the
public Python face only, timed with HIP events.

  python tools/bench_conv.py [--seconds 3600] [--out profiles/conv_bench.jsonl]

One child process per step, each under its own time limit; a step that fails
or runs out of time ends the run (nothing more is started on the GPU).  Steps:
T in {4096, 48000, 240000} taps, each with a warm-up; the yardsticks: the
existing 1024-tap overlap-save FIR (Plugin.fir) over the same hour, and the
float64 FFT convolution on the CPU (numpy, 60 s of stereo scaled to the hour).
One JSON line per step.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dsp-bench_amd"))


def gpu_step(kind: str, T: int, seconds: int, reps: int) -> dict:
    import numpy as np
    import torch
    import dspbench as d
    L, B, C = 48000 * seconds, 512, 2
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((C, L), generator=g, device="cuda") * 2 - 1
    taps = (np.random.default_rng(1).standard_normal(T) / np.sqrt(T)).astype(np.float32)
    plug = d.Plugin.conv(taps) if kind == "conv" else d.Plugin.fir(taps)
    out = torch.empty((C, (L + B - 1) // B * B), device="cuda")
    d.render_offline(x, C, B, 48000.0, plug, out=out)   # warm-up: table, scratch
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d.render_offline(x, C, B, 48000.0, plug, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    r = {"step": f"{kind}{T}", "taps": T, "seconds": seconds, "channels": C, "ms": sorted(ms),
         "ms_median": float(np.median(ms)), "audio_bytes": 2 * C * L * 4}
    if kind == "conv":
        p, f, b = d.conv_plan(T, L, B, C)
        r.update(partitions=p, frames=f, scratch_bytes=b,
                 mac_algorithmic_bytes=2 * C * f * 33792 + p * 33792)  # X and Y spectra once each, plus H
    return r


def cpu_step(T: int, seconds: int) -> dict:
    import numpy as np
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from convutil import conv_f64
    sec = min(seconds, 60)
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (2, 48000 * sec))
    taps = rng.standard_normal(T) / np.sqrt(T)
    t0 = time.perf_counter()
    for c in range(2):
        conv_f64(x[c], taps, x.shape[1])
    dt = (time.perf_counter() - t0) * 1e3
    return {"step": f"cpu_f64_fft{T}", "taps": T, "seconds_measured": sec, "ms_measured": dt,
            "ms_scaled_to_call": dt * seconds / sec, "threads": int(os.environ.get("OMP_NUM_THREADS", "1"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "conv_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=240, help="time limit of each step, seconds")
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        kind, T = a.child[0], int(a.child[1])
        r = cpu_step(T, a.seconds) if kind == "cpu" else gpu_step(kind, T, a.seconds, a.reps)
        print("RESULT " + json.dumps(r))
        return 0
    steps = [("conv", 4096), ("conv", 48000), ("conv", 240000), ("fir", 1024), ("cpu", 4096), ("cpu", 240000)]
    lines = []
    for kind, T in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--seconds", str(a.seconds), "--reps", str(a.reps),
               "--child", kind, str(T)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"step {kind}{T}: time limit of {a.limit} s; stopping", file=sys.stderr)
            break
        res = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(f"step {kind}{T}: exit {p.returncode}; stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            break
        print(res[0], flush=True)
        lines.append(res[0])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("".join(ln + "\n" for ln in lines))
    return 0 if len(lines) == len(steps) else 1


if __name__ == "__main__":
    sys.exit(main())
