"""dsp_pvoc and dsp_time_stretch on one hour of 48 kHz stereo at hop 2048, run by
hand (not bench.py's workload): the median of 5 timed calls at rates 0.8, 1.0
and 1.25 of dsp_pvoc alone, of dsp_time_stretch end to end, of dsp_stft from
the same build (the yardstick: a store-bound launch of the same layout), and of
the same recurrence written in torch on the same device (angle, a float64
cumsum, polar).  dsp_pvoc's line counts the bytes the call must move -- the
input spectrogram read once, the output written once -- and the fraction of
8 TB/s that is; the call reads its input twice (the sums launch and the frames
launch), which `bytes_moved` counts.

    python tools/bench_pvoc.py [--seconds 3600] [--out profiles/pvoc_bench.jsonl]

One JSON line per measurement is printed and appended to --out.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dsp-bench_amd"))

PEAK = 8e12  # bytes / s


def timed(torch, fn, reps=5, warmup=2):
    for _ in range(warmup):
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


def torch_pvoc(torch, Z, rate, Fo):
    """The same recurrence in torch: angle, cumsum in float64, polar."""
    s = torch.arange(Fo, dtype=torch.float64, device=Z.device) * rate
    f = s.floor().long()
    a = (s - f).float()[None, :, None]
    Zp = torch.cat([Z, torch.zeros_like(Z[:, :2])], dim=1)
    z0, z1 = Zp[:, f], Zp[:, f + 1]
    mag = (1 - a) * z0.abs() + a * z1.abs()
    inc = torch.angle(z1 * z0.conj()).double()
    phase = torch.angle(Z[:, :1]).double() + torch.cumsum(inc, dim=1) - inc
    return torch.polar(mag, phase.float())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--hop", type=int, default=2048)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pvoc_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import dspbench as d

    C, L, H, K = 2, 48000 * a.seconds, a.hop, 4097
    F = d.stft_plan(L, C, H)["frames"]
    x = torch.empty((C, L), device="cuda").uniform_(-1, 1)
    Z = torch.empty((C, F, K), dtype=torch.complex64, device="cuda")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        def emit(name, rate, med, ms, nbytes, **more):
            line = {"what": name, "device": torch.cuda.get_device_name(0), "channels": C, "samples": L, "hop": H,
                    "rate": rate, "frames_in": F, "median_ms": round(med, 4), "runs_ms": [round(v, 4) for v in ms],
                    "bytes": nbytes, "fraction_of_8TBps": round(nbytes / (med * 1e-3) / PEAK, 4), **more}
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")
            f.flush()

        med, ms = timed(torch, lambda: d.stft(x, H, "hann", out=Z))
        emit("dsp_stft", None, med, ms, 4 * C * L + 8 * C * F * K)
        for rate in (0.8, 1.0, 1.25):
            Fo = d.pvoc_plan(F, rate, C)["frames"]
            out = torch.empty((C, Fo, K), dtype=torch.complex64, device="cuda")
            med, ms = timed(torch, lambda: d.phase_vocoder(Z, rate, out=out))
            used = min(F, int((Fo - 1) * rate) + 2)  # input frames the output reads
            emit("dsp_pvoc", rate, med, ms, 8 * C * K * (used + Fo), frames_out=Fo,
                 bytes_moved=8 * C * K * (2 * used + Fo))
            if not a.no_torch:
                med, ms = timed(torch, lambda: torch_pvoc(torch, Z, rate, Fo), reps=5, warmup=1)
                emit("torch angle/cumsum64/polar", rate, med, ms, 8 * C * K * (used + Fo), frames_out=Fo)
            del out
            torch.cuda.empty_cache()
            p = d.time_stretch_plan(L, rate, C, H)
            y = torch.empty((C, p["Lout"]), device="cuda")
            med, ms = timed(torch, lambda: d.time_stretch(x, rate, H, out=y), reps=5, warmup=1)
            emit("dsp_time_stretch", rate, med, ms, 4 * C * (L + p["Lout"]), frames_out=p["frames_out"],
                 samples_out=p["Lout"], device_bytes=p["device_bytes"])
            del y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
