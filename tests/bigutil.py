"""Expectations for calls at positions past 2^32: sample offsets, cursors,
row lengths and byte offsets that no longer fit 32 bits (used by
test_gpu_large_positions.py, pinned against the oracle at small sizes by
test_large_positions_cpu.py).

Everything here is Python-integer or numpy arithmetic: no expectation is
computed by the library under test.

  offsets(B)       the sample offsets of the large-position cases, each with
                   the nearest multiple of B at or above it (the calls refuse
                   anything else: dsp_exec.sample_offset in dspbench.h)
  ramp_slice       a per-sample map depends on the position only through
                   (O + i) mod B, so a B-periodic render at offset O is the
                   render at offset 0 of a file B samples longer, from sample
                   r = O mod B on
  loop_index       the file index of output sample i in loop mode
  pixel_of,        the display reductions' sample -> pixel rule and its
  pixel_first      inverse, in unbounded integers
  planted, minmax_expect   a zero row with a few planted values and the
                   (max, min) per pixel it must give
"""
import numpy as np

P31, P32, P40, P53 = 1 << 31, 1 << 32, 1 << 40, 1 << 53

# offsets no call accepts at the block sizes used (none divides them): an even
# and an odd one (goff % 2 chooses fused or unfused in dsp_render_stft)
UNALIGNED = (P32 + 778, P32 + 777)


def offsets(B):
    """[(name, O)]: 2^32 - 2B (the call crosses 2^32 inside its rows), 2^32,
    2^32 + 3B, 2^40 + B, 2^53 - 4B."""
    return [("2^32-2B", P32 - 2 * B), ("2^32", P32), ("2^32+3B", P32 + 3 * B), ("2^40+B", P40 + B),
            ("2^53-4B", P53 - 4 * B)]


def aligned_up(O, B):
    """The smallest multiple of B that is >= O."""
    return -(-O // B) * B


def accepted_offsets(B):
    """[(name, O')]: offsets(B) moved up to a multiple of B (unchanged for a
    power-of-two B <= 2^32), without duplicates.  2^32 - 2B moved up by less
    than B still lies more than B below 2^32."""
    seen, out = set(), []
    for name, O in offsets(B):
        A = aligned_up(O, B)
        if A not in seen:
            seen.add(A)
            out.append((name if A == O else f"{name}->{A}", A))
    return out


def refused_offsets(B):
    """The listed offsets that are no multiple of B, and the two unaligned ones."""
    return [O for _, O in offsets(B) if O % B] + [O for O in UNALIGNED if O % B]


def phase(O, B):
    return int(O) % int(B)


def ramp_slice(ref, O, B, n):
    """ref: [C, >= n + B) rendered at offset 0 -> the n samples a call at
    offset O must give."""
    r = phase(O, B)
    assert ref.shape[-1] >= r + n
    return ref[..., r:r + n]


def loop_index(cursor, i0, i1, L):
    """File indices of the output samples [i0, i1) of a loop render (int64)."""
    return (np.arange(i0, i1, dtype=np.int64) + int(cursor)) % int(L)


def pixel_of(s, P, n):
    """The pixel of sample s of n in P pixels (opengl.h:877-890 in 64 bits)."""
    return int(s) * int(P) // int(n)


def pixel_first(p, P, n):
    """The first sample (or frame) of pixel p: ceil(p n / P)."""
    return -(-int(p) * int(n) // int(P))


def boundary_samples(n, P, pixels):
    """The two samples on each side of the start of each pixel in `pixels`."""
    out = []
    for p in pixels:
        s = pixel_first(p, P, n)
        out += [s - 2, s - 1, s, s + 1]
    return [s for s in out if 0 <= s < n]


def fixed_positions(n):
    """0, 2^31 +- 1, 2^32 - 1, 2^32, 2^32 + 1 (scaled to n when n is small:
    halves and the last quarter) and n - 1."""
    if n > P32 + 1:
        pos = [0, P31 - 1, P31 + 1, P32 - 1, P32, P32 + 1, n - 1]
    else:
        h, q = n // 2, n - n // 4
        pos = [0, h - 1, h + 1, q - 1, q, q + 1, n - 1]
    return pos


def planted(n, Ps=(1920,), pixels=lambda P: (1, P // 3, P - 1)):
    """{sample: value}: distinct values in (-1, 1), signs alternating, at
    fixed_positions(n) and around three pixel boundaries of every P in Ps."""
    pos = list(fixed_positions(n))
    for P in Ps:
        pos += boundary_samples(n, P, pixels(P))
    pos = sorted(set(pos))
    vals = {}
    for k, s in enumerate(pos):
        v = np.float32((0.05 + 0.9 * (k + 1) / (len(pos) + 1)) * (1 if k % 2 == 0 else -1))
        vals[s] = v
    return vals


def minmax_expect(vals, n, P):
    """(vmax [P], vmin [P]) float32 of a zero row of n samples holding vals:
    an untouched pixel is (0, 0); a planted pixel holds its largest value where
    positive and its smallest where negative."""
    vmax, vmin = np.zeros(P, np.float32), np.zeros(P, np.float32)
    for s, v in vals.items():
        p = pixel_of(s, P, n)
        vmax[p] = max(vmax[p], v)
        vmin[p] = min(vmin[p], v)
    return vmax, vmin


def first_row_past(nbytes, ld):
    """The first row of ld floats that starts at or past byte `nbytes`."""
    return -(-int(nbytes) // (4 * int(ld)))
