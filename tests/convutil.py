"""Float64 reference for DSP_PLUGIN_CONV's tests: y[n] = sum_k taps[k] x[n - k]
by one float64 FFT, so that long filters do not cost O(L T)
(test_conv_plan.py pins it to oracle.fir_f64)."""
import numpy as np


def conv_f64(x, taps, Ly: int) -> np.ndarray:
    """The first Ly samples of x * taps in float64 (zero past the signal)."""
    x = np.asarray(x, np.float64)
    h = np.asarray(taps, np.float64)
    if x.size == 0:
        return np.zeros(Ly)
    n = 1
    while n < x.size + h.size - 1:
        n *= 2
    y = np.fft.irfft(np.fft.rfft(x, n) * np.fft.rfft(h, n), n)[:min(Ly, x.size + h.size - 1)]
    out = np.zeros(Ly)
    out[:y.size] = y
    return out


def conv_inputs(seed: int, C: int, L: int, T: int):
    """The tests' signals: x uniform in [-1, 1], taps randn(T) / sqrt(T), float32."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (C, L)).astype(np.float32)
    taps = (rng.standard_normal(T) / np.sqrt(T)).astype(np.float32)
    return x, taps
