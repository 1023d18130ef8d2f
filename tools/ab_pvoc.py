"""The A/B runs behind dsp_pvoc's four design choices, run by hand
on the device: every side through the library's own kernels, switched by the
test hooks DSP_DEBUG_PVOC_CHUNK and DSP_DEBUG_PVOC_VARIANT.

  chunk     16, 32, 64 (the product), 128, 256, 1024 output frames per chunk
  variant   0 the product (increments as differences of argument words, recomputed
            by the frames launch, polynomial cos / sin); 1 one argument of the
            product Z[f + 1] conj Z[f] per output frame; 2 the hardware's
            turn-based cos / sin; 4 the increments stored by the sums launch
            and read back by the frames launch

For each side: the median of 5 timed dsp_pvoc calls on one hour of 48 kHz stereo
at hop 2048 at rates 0.8, 1.0 and 1.25, and (where the values change: variants 1
and 2) the worst ratio against pvoc64 over tests/pvocutil.py's cases, the same
measurement as GPU_RATIO.  Then ten more dsp_time_stretch calls at rate 1.25
with each one's time, to see whether a slow call comes back.

    python tools/ab_pvoc.py [--seconds 3600] [--out profiles/pvoc_ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "dsp-bench_amd"), os.path.join(REPO, "tools"), os.path.join(REPO, "tests")]

CHUNK_HOOK, VARIANT_HOOK = 7, 8
SIDES = [(64, 0), (16, 0), (32, 0), (128, 0), (256, 0), (1024, 0), (64, 1), (64, 2), (64, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pvoc_ab.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import dspbench as d
    from dspbench import _lib as L
    import pvoc_model as pm
    import pvocutil as pu
    from bench_pvoc import timed

    lib = L.lib()
    C, Ls, H, K = 2, 48000 * a.seconds, 2048, 4097
    F = d.stft_plan(Ls, C, H)["frames"]
    x = torch.empty((C, Ls), device="cuda").uniform_(-1, 1)
    Z = d.stft(x, H, "hann")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        def emit(line):
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")
            f.flush()

        for chunk, variant in SIDES:
            L.check(lib.dsp_debug_set(CHUNK_HOOK, 0 if chunk == 64 else chunk), "dsp_debug_set")
            L.check(lib.dsp_debug_set(VARIANT_HOOK, variant), "dsp_debug_set")
            line = {"what": "dsp_pvoc A/B", "chunk": chunk, "variant": variant, "frames_in": F}
            if variant in (0, 1, 2) and chunk == 64:
                line["worst_ratio"] = max(
                    pm.ratio(d.phase_vocoder(torch.from_numpy(np.array(pu.make_spectrum(c))).cuda(), c.rate).cpu().numpy(),
                             pu.reference(c)) for c in pu.CASES)
            for rate in (0.8, 1.0, 1.25):
                Fo = d.pvoc_plan(F, rate, C)["frames"]
                out = torch.empty((C, Fo, K), dtype=torch.complex64, device="cuda")
                med, ms = timed(torch, lambda: d.phase_vocoder(Z, rate, out=out))
                line[f"ms_at_{rate}"] = round(med, 4)
                del out
                torch.cuda.empty_cache()
            emit(line)
        L.check(lib.dsp_debug_set(CHUNK_HOOK, 0), "dsp_debug_set")
        L.check(lib.dsp_debug_set(VARIANT_HOOK, 0), "dsp_debug_set")
        del Z
        torch.cuda.empty_cache()
        p = d.time_stretch_plan(Ls, 1.25, C, H)
        y = torch.empty((C, p["Lout"]), device="cuda")
        ms = []
        for _ in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.time_stretch(x, 1.25, H, out=y)
            torch.cuda.synchronize()
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        emit({"what": "dsp_time_stretch, ten calls", "rate": 1.25, "wall_ms": ms, "median_ms": statistics.median(ms),
              "device_bytes": p["device_bytes"]})


if __name__ == "__main__":
    main()
