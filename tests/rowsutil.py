"""Row layouts for the C ABI's `float *` per channel: a [C, n] view (torch
CUDA or numpy) inside one larger allocation, so that a test chooses where each
row starts relative to a 16-byte boundary, what lies between the rows, and can
tell afterwards what a call touched.

The allocation starts on a 16-byte boundary.  Row c starts at float
G + off[c] + c * pitch, pitch = roundup4(n + G + 3) + stride_mod, so with
stride_mod = 0 it sits off[c] floats (0..3) past a 16-byte boundary and with
stride_mod = 1 the boundary offset advances by one float per row.  At least
G = 64 floats of guard lie before and after every row.  The rows are one
strided view, so off is a constant or an arithmetic sequence (0, 1, 2).

Everything -- rows and guards -- is filled with one NaN bit pattern, SENTINEL.
  output rows  check_output(): every word outside the written region still
               holds SENTINEL (compared as int32, not as floats) and no word
               inside it does (a sample the kernel never wrote is caught).
  input rows   fill() writes the L samples the call is told about; what
               follows them, and the guards, stay NaN.  The operations under
               test are finite for finite input, so assert_finite() on the
               outputs fails exactly when a sample outside [0, L) was consumed.
"""
import numpy as np

G = 64
SENTINEL = np.int32(0x7FC5A5A5)  # a quiet NaN no kernel here produces

# name: (input offsets, output offsets, stride_mod)
LAYOUTS = {
    "base": (0, 0, 0),
    "in1": (1, 0, 0),
    "out1": (0, 1, 0),
    "both2": (2, 2, 0),          # 8-byte but not 16-byte aligned
    "in3_out1": (3, 1, 0),
    "mixed": ((0, 1, 2), (0, 1, 2), 0),   # one group of aligned and unaligned rows
    "odd_stride": (0, 0, 1),     # what a dense [C, L] tensor with L = 1 (mod 4) gives
}
ALL = tuple(LAYOUTS)
FEW = ("base", "in1", "out1", "mixed")


def offsets(off, C):
    """off as a tuple of C row offsets (a tuple longer than C is cut)."""
    t = tuple(off[:C]) if isinstance(off, (tuple, list)) else (int(off),) * C
    assert len(t) == C and all(0 <= o <= 3 for o in t), (off, C)
    return t


class Rows:
    """C rows of n floats in one SENTINEL-filled allocation.  `view` is the
    [C, n] buffer to hand to the library; torch=None makes host (numpy) rows."""

    def __init__(self, C, n, off=0, stride_mod=0, torch=None):
        self.C, self.n, self.torch = C, n, torch
        self.off = offsets(off, C)
        pitch = (n + G + 3 + 3) // 4 * 4 + stride_mod
        self.starts = [G + self.off[c] + c * pitch for c in range(C)]
        step = self.starts[1] - self.starts[0] if C > 1 else pitch
        assert all(self.starts[c] == self.starts[0] + c * step for c in range(C)), "offsets must be arithmetic"
        total = (self.starts[-1] + n if C else G) + G
        if torch is not None:
            self.whole = torch.full((total,), int(SENTINEL), dtype=torch.int32, device="cuda").view(torch.float32)
            assert self.whole.data_ptr() % 16 == 0
            self.view = self.whole.as_strided((C, n), (step, 1), self.starts[0] if C else 0)
        else:
            raw = np.full(total + 4, SENTINEL, np.int32).view(np.float32)
            skip = (-raw.ctypes.data % 16) // 4
            self.whole = raw[skip:skip + total]
            self.view = np.lib.stride_tricks.as_strided(self.whole[self.starts[0] if C else 0:], (C, n),
                                                        (step * 4, 4))

    def ptrs(self):
        if self.torch is not None:
            return [self.view[c].data_ptr() for c in range(self.C)]
        return [self.view[c].ctypes.data for c in range(self.C)]

    def frames(self, F, ld):
        """The rows as [C, F, ld] (n = F ld): magnitude rows of ld floats."""
        assert F * ld == self.n
        if self.torch is not None:
            return self.view.unflatten(1, (F, ld))
        return np.lib.stride_tricks.as_strided(self.view, (self.C, F, ld), (self.view.strides[0], ld * 4, 4))

    def fill(self, x, L=None):
        """The call's L samples of every row (x: numpy [C, >= L]); the rest stays NaN."""
        x = np.asarray(x, np.float32)
        L = x.shape[1] if L is None else L
        assert x.shape[0] == self.C and L <= self.n
        if self.torch is not None:
            self.view[:, :L] = self.torch.from_numpy(np.ascontiguousarray(x[:, :L])).cuda()
        else:
            self.view[:, :L] = x[:, :L]
        return self

    def words(self):
        """The whole allocation as int32 on the host."""
        if self.torch is not None:
            return self.whole.view(self.torch.int32).cpu().numpy()
        return self.whole.view(np.int32).copy()

    def numpy(self, n=None):
        """The rows' first n floats, a dense host copy."""
        w = self.words().view(np.float32)
        n = self.n if n is None else n
        return np.stack([w[s:s + n] for s in self.starts]) if self.C else np.zeros((0, n), np.float32)

    def written_mask(self, Ly, K=None, ld=None):
        """The words a call must write: [0, Ly) of every row; with K and ld,
        columns [0, K) of each row of ld floats inside it."""
        m = np.zeros(self.whole.shape[0], bool)
        for s in self.starts:
            if K is None:
                m[s:s + Ly] = True
            else:
                assert Ly % ld == 0
                m[s:s + Ly].reshape(-1, ld)[:, :K] = True
        return m

    def check_guards(self, Ly=None, K=None, ld=None):
        """Every word outside the written region still holds SENTINEL."""
        w, m = self.words(), self.written_mask(self.n if Ly is None else Ly, K, ld)
        bad = np.flatnonzero(~m & (w != SENTINEL))
        assert bad.size == 0, f"{bad.size} words written outside the rows, the first at float {bad[0]} " \
                              f"(rows start at {self.starts}, n = {self.n})"

    def check_written(self, Ly=None, K=None, ld=None):
        """No word of the written region still holds SENTINEL."""
        w, m = self.words(), self.written_mask(self.n if Ly is None else Ly, K, ld)
        bad = np.flatnonzero(m & (w == SENTINEL))
        assert bad.size == 0, f"{bad.size} output words never written, the first at float {bad[0]} " \
                              f"(rows start at {self.starts}, n = {self.n})"

    def check_output(self, Ly=None, K=None, ld=None):
        self.check_guards(Ly, K, ld)
        self.check_written(Ly, K, ld)


def assert_finite(*arrays):
    """A NaN or Inf in an output: a sample outside [0, L) of an input row was consumed."""
    for a in arrays:
        a = np.asarray(a)
        bad = np.flatnonzero(~np.isfinite(a.reshape(-1)))
        assert bad.size == 0, f"{bad.size} non-finite outputs, the first at flat index {bad[0]} of shape {a.shape}"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
