"""conv_model.py -- float32 model of DSP_PLUGIN_CONV (csrc/conv_fdl.hip): uniform
partitioned overlap-save on 8192-point real frames with torch.fft on the CPU.

  partitions of 4096 taps, H_p = FFT_8192(partition zero-padded) in float64,
      rounded once to fp32 (host_tables.cpp conv_table)
  frame f = input [4096 (f - 1), 4096 (f + 1)), zero outside [0, L)
  X_f = rfft(frame) in fp32;  Y_f = sum_p H_p X_{f-p}, accumulated in fp32 in
      the kernel's order (oldest frame first);  y[4096 f ..) = upper half of
      irfft(Y_f)

The index math is the kernel's; the transforms are torch's, so the rounding is
a float32 FFT's and not bit for bit the kernel's.  Run as a script it prints
the worst max|y - y64| / max|y64| over the shapes of tests/test_gpu_conv.py:
one of the two measurements the tests' tolerance is derived from.
"""
import os
import sys

import numpy as np
import torch

HOP, N = 4096, 8192


def conv_model(x, taps, Ly: int) -> np.ndarray:
    """x: float32 [L]; taps: float32 [T]; returns float32 [Ly]."""
    x = np.asarray(x, np.float32)
    taps = np.asarray(taps, np.float32)
    P = -(-taps.size // HOP)
    F = -(-Ly // HOP)
    hp = np.zeros((P, N), np.float64)
    for p in range(P):
        part = taps[p * HOP:(p + 1) * HOP]
        hp[p, :part.size] = part
    H = torch.from_numpy(np.fft.rfft(hp, axis=1).astype(np.complex64))   # rounded once
    xp = np.zeros((F + 1) * HOP, np.float32)                               # x[-4096 ..), zero-padded
    n = min(x.size, F * HOP)
    xp[HOP:HOP + n] = x[:n]
    frames = torch.from_numpy(np.stack([xp[f * HOP:f * HOP + N] for f in range(F)]))
    X = torch.fft.rfft(frames, dim=1)                                      # complex64
    Y = torch.zeros_like(X)
    for p in range(P - 1, -1, -1):                                         # oldest frame first
        if p < F:
            Y[p:] += H[p] * X[:F - p]
    y = torch.fft.irfft(Y, n=N, dim=1)[:, HOP:].reshape(-1).numpy()
    return y[:Ly].astype(np.float32)


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "tests"))
    from convutil import conv_f64, conv_inputs
    shapes = [(T, Lx, B) for T in (2049, 4096, 4097, 8193, 40_000, 70_001)
              for Lx, B in ((100, 100), (4096, 512), (4097, 1), (12_289, 100), (70_001, 512))]
    shapes.append((1 << 18, 300_000, 512))
    worst = 0.0
    for i, (T, Lx, B) in enumerate(shapes):
        x, taps = conv_inputs(i, 1, Lx, T)
        Ly = -(-Lx // B) * B
        y64 = conv_f64(x[0], taps, Ly)
        ratio = float(np.max(np.abs(conv_model(x[0], taps, Ly) - y64)) / np.max(np.abs(y64)))
        worst = max(worst, ratio)
        print(f"T={T:7d} partitions={-(-T // HOP):3d} L={Lx:7d} B={B:4d}  max|y-y64|/max|y64| = {ratio:.3e}")
    print(f"worst ratio: {worst:.3e}")


if __name__ == "__main__":
    main()
