"""dsp_stft / dsp_istft on one hour of 48 kHz stereo at hop 4096, run by hand
(not bench.py's workload): the median of 5 timed calls each of dsp_stft,
dsp_istft and the round trip, beside dsp_stft_magnitude from the same build and
torch.stft / torch.istft on the same device.  Each line gives the bytes the
call must move (input read once, output written once; for dsp_istft also the
scratch written and read once) and the fraction of 8 TB/s that is.  That
fraction is nominal for dsp_istft: a chunk's scratch (64 MiB) is counted as
memory traffic although it may well stay in the last-level cache.  The library's
calls run with the Hann window, torch's with Hamming, because torch.istft
refuses a window whose overlap-added envelope reaches zero (Hann's ends at
center=False); the window's values do not change the cost of either.

    python tools/bench_stft.py [--seconds 3600] [--out profiles/stft_cx_bench.jsonl]

One JSON line per measurement is printed and appended to --out.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dsp-bench_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--hop", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stft_cx_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import dspbench as d
    import stft_model as sm

    C, L, H, N, K = 2, 48000 * a.seconds, a.hop, 8192, 4097
    F = d.stft_plan(L, C, H)["frames"]
    Lout = d.istft_plan(F, C, H)["Lout"]
    x = torch.empty((C, L), device="cuda").uniform_(-1, 1)
    Z = torch.empty((C, F, K), dtype=torch.complex64, device="cuda")
    y = torch.empty((C, Lout), device="cuda")
    mag = d.stft_magnitude(x, N, H, d.DSP_WIN_HANN)
    w = torch.from_numpy(sm.window_table("hamming")).cuda()
    in_b, spec_b, mag_b, out_b = 4 * C * L, 8 * C * F * K, 4 * C * F * K, 4 * C * Lout
    scratch_b = 2 * 4 * C * F * N

    def t_stft():
        return torch.stft(x, N, H, window=w, center=False, return_complex=True)

    T = t_stft()
    runs = [
        ("dsp_stft", lambda: d.stft(x, H, "hann", out=Z), in_b + spec_b),
        ("dsp_istft", lambda: d.istft(Z, H, "hann", out=y), spec_b + scratch_b + out_b),
        ("round_trip", lambda: d.istft(d.stft(x, H, "hann", out=Z), H, "hann", out=y), in_b + 2 * spec_b + scratch_b + out_b),
        ("dsp_stft_magnitude", lambda: d.stft_magnitude(x, N, H, d.DSP_WIN_HANN, out=mag), in_b + mag_b),
        ("torch.stft", t_stft, in_b + spec_b),
        ("torch.istft", lambda: torch.istft(T, N, H, window=w, center=False), spec_b + out_b),
    ]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for name, fn, nbytes in runs:
            med, ms = timed(torch, fn)
            line = {"what": name, "device": torch.cuda.get_device_name(0), "channels": C, "samples": L, "hop": H,
                    "frames": F, "median_ms": round(med, 4), "runs_ms": [round(v, 4) for v in ms], "bytes": nbytes,
                    "fraction_of_8TBps": round(nbytes / (med * 1e-3) / PEAK, 4)}
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
