"""loudness_model.py -- dsp_loudness on the CPU, for the tolerance and the
timing figures of DESIGN 4.5c.

  python tools/loudness_model.py tol    the serial fp32 chain (oracle.biquad_f32, squares summed in
                                        float64) against the float64 model over the shapes of
                                        tests/test_gpu_loudness.py: worst hop-energy ratio (MODEL32)
  python tools/loudness_model.py time   the float64 model on one core, 10 s of stereo at 48 kHz
  python tools/loudness_model.py ebu    EBU Tech 3341's two sine cases through the model
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("dsp-bench_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))

import loudnessutil as lu  # noqa: E402


def ratio(z, z64):
    return float(np.max(np.abs(z - z64)) / max(float(np.max(z64)), 1e-300)) if z64.size else 0.0


def tol():
    import test_gpu_loudness as tg
    worst = 0.0
    for sr, Lx in tg.hop_cases():
        x = lu.noise(tg.seed_of(sr, Lx), 1, Lx)[0]
        r = ratio(lu.hop_energy32(x, sr), lu.hop_energy64(x, sr))
        worst = max(worst, r)
        print(f"sr={sr} L={Lx}: {r:.3e}")
    x = lu.noise(77, 17, 14 * 2048 + 5)
    for Cn, Lx in tg.channel_cases():
        for c in range(Cn):
            r = ratio(lu.hop_energy32(x[c, :Lx], tg.CHANNEL_RATE), lu.hop_energy64(x[c, :Lx], tg.CHANNEL_RATE))
            worst = max(worst, r)
    for sr, Cn, Lx in tg.long_cases():
        xl = lu.noise(tg.seed_of(sr, Lx) + 5, Cn, Lx)
        for c in range(Cn):
            r = ratio(lu.hop_energy32(xl[c], sr), lu.hop_energy64(xl[c], sr))
            worst = max(worst, r)
            print(f"sr={sr} C={Cn} c={c} L={Lx}: {r:.3e}")
    print(f"serial fp32 chain, worst hop-energy ratio: {worst:.3e}")


def timing(seconds=10):
    x = lu.noise(0, 2, 48000 * seconds)
    t0 = time.perf_counter()
    m = lu.loudness64(x, 48000)
    dt = (time.perf_counter() - t0) * 1e3
    print(f"float64 model, {seconds} s of stereo at 48 kHz on one core: {dt:.1f} ms "
          f"({dt * 3600 / seconds / 1e3:.1f} s for an hour), integrated {m['integrated']:.3f} LUFS")
    return dt


def ebu():
    for x, what in ((lu.sine(48000, 3, 1000.0, -23.0, 2), "stereo 1 kHz at -23 dBFS"),
                    (lu.sine(48000, 3, 997.0, 0.0, 1), "mono 997 Hz at 0 dBFS")):
        print(f"{what}: {lu.loudness64(x, 48000)['integrated']:.3f} LUFS")


if __name__ == "__main__":
    {"tol": tol, "time": timing, "ebu": ebu}[sys.argv[1] if len(sys.argv) > 1 else "tol"]()
