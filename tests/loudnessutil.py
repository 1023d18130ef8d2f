"""The float64 numpy model of dsp_loudness (include/dspbench/dspbench.h):
K-weighting coefficients from the formulas, hop energies through the oracle's
float64 cascade, BS.1770-4 gating and the EBU Tech 3342 range.  Nothing shared
with the library."""
import numpy as np

import oracle

# ITU-R BS.1770-4, table of the two stages at 48 kHz
BS1770_48K = [[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
              [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]]


def kcoef64(sr):
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    s1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
          2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    s2 = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([s1, s2], np.float64)


def kcoef(sr):
    """The coefficients as the library rounds them: once, to float32."""
    return kcoef64(sr).astype(np.float32)


def plan(sr, L=0):
    hop = (sr + 5) // 10
    return dict(hop=hop, hops=L // hop, oversample=4 if sr < 88200 else 2 if sr < 176400 else 1)


def _hop_sums(y, hop):
    hops = y.size // hop
    return (np.asarray(y[:hops * hop], np.float64) ** 2).reshape(hops, hop).sum(axis=1)


def hop_energy64(x, sr):
    """z[j] of one channel: float64 cascade over the float32-rounded coefficients."""
    y, _ = oracle.biquad_f64(np.asarray(x, np.float32), kcoef(sr))
    return _hop_sums(y, plan(sr)["hop"])


def hop_energy32(x, sr):
    """The serial fp32 chain, its squares summed in float64 (MODEL32)."""
    return _hop_sums(oracle.biquad_f32(np.asarray(x, np.float32), kcoef(sr)), plan(sr)["hop"])


def lufs(w):
    w = np.asarray(w, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(w > 0, -0.691 + 10.0 * np.log10(np.where(w > 0, w, 1.0)), -np.inf)


def block_powers(z, hop, n, weights=None):
    """w_i over blocks of n hops: sum_c G_c (z[c][i] + .. + z[c][i + n - 1]) / (n hop)."""
    z = np.atleast_2d(np.asarray(z, np.float64))
    g = np.ones(z.shape[0]) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    e = (g[:, None] * z).sum(axis=0)
    if e.size < n:
        return np.zeros(0)
    return np.array([e[i:i + n].sum() for i in range(e.size - n + 1)]) / (n * hop)


def gate(z, hop, weights=None):
    """The four loudness fields and the two counts, plus `margin`: the least
    distance (LU) of a momentary block's loudness from either gate."""
    wm = block_powers(z, hop, 4, weights)
    lm = lufs(wm)
    out = dict(blocks=int(wm.size), gated_blocks=0, integrated=-np.inf, range=0.0, margin=np.inf,
               momentary_max=float(lm.max()) if lm.size else -np.inf)
    if lm.size:
        out["margin"] = float(np.min(np.abs(lm - -70.0)))
    a = lm > -70.0
    if a.any():
        rel = -0.691 + 10.0 * np.log10(wm[a].mean()) - 10.0
        out["margin"] = min(out["margin"], float(np.min(np.abs(lm - rel))))
        b = a & (lm > rel)
        if b.any():
            out["integrated"] = float(-0.691 + 10.0 * np.log10(wm[b].mean()))
            out["gated_blocks"] = int(b.sum())
            out["gated_mean"] = float(wm[b].mean())
    ws = block_powers(z, hop, 30, weights)
    ls = lufs(ws)
    out["short_term_max"] = float(ls.max()) if ls.size else -np.inf
    a = ls > -70.0
    if a.any():
        rel = -0.691 + 10.0 * np.log10(ws[a].mean()) - 20.0
        s = np.sort(ls[a & (ls > rel)])
        n = s.size
        if n:
            out["range"] = float(s[int((n - 1) * 0.95 + 0.5)] - s[int((n - 1) * 0.10 + 0.5)])
    return out


def loudness64(x, sr, weights=None):
    """The whole model: hop energies [C, hops] and gate()'s fields."""
    x = np.atleast_2d(np.asarray(x, np.float32))
    z = np.stack([hop_energy64(x[c], sr) for c in range(x.shape[0])])
    out = gate(z, plan(sr)["hop"], weights)
    out["hop_energy"] = z
    return out


def sine(sr, seconds, freq, dbfs, channels=1, phase=0.0):
    n = np.arange(int(round(sr * seconds)), dtype=np.float64)
    s = (10.0 ** (dbfs / 20.0) * np.sin(2.0 * np.pi * freq * n / sr + phase)).astype(np.float32)
    return np.tile(s, (channels, 1))


def noise(seed, C, L, amp=1.0):
    """Uniform noise in [-amp, amp], one seed per channel."""
    return np.stack([(amp * np.random.default_rng(seed + 1000 * c).uniform(-1, 1, L)).astype(np.float32)
                     for c in range(C)])
