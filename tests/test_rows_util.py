"""rowsutil on the host: the layouts are what their names say, and each of the
three checks (guards intact, every output word written, nothing read past L)
catches a fake kernel that is wrong by one word."""
import numpy as np
import pytest

import rowsutil as ru


def fake_gain(xin, out, L, Ly, read=None, write=None):
    """out[c][0:Ly) = 2 x[c][0:L), zero padded -- a correct 'kernel' on row
    pointers; read / write override how many words it touches."""
    for c in range(out.shape[0]):
        n = L if read is None else read
        o = Ly if write is None else write
        row = np.lib.stride_tricks.as_strided(out[c], (o,), (4,))     # (may run past the view, as a kernel can)
        src = np.lib.stride_tricks.as_strided(xin[c], (n,), (4,))
        row[:] = 0.0
        row[:min(n, o)] = 2.0 * src[:min(n, o)]
        if n > L:   # a tile that sums one sample too many
            row[0] += src[n - 1]


def buffers(layout, C=3, L=1001, Ly=1024):
    io, oo, sm = ru.LAYOUTS[layout]
    x = np.random.default_rng(1).uniform(-1, 1, (C, L)).astype(np.float32)
    return x, ru.Rows(C, L, io, sm).fill(x), ru.Rows(C, Ly, oo, sm)


@pytest.mark.parametrize("layout", ru.ALL)
def test_layout_offsets_and_strides(layout):
    io, oo, sm = ru.LAYOUTS[layout]
    C, n = 3, 1001
    for off in (io, oo):
        r = ru.Rows(C, n, off, sm)
        want = ru.offsets(off, C)
        p = r.ptrs()
        pitch = (p[1] - p[0]) // 4 - (want[1] - want[0])
        assert pitch % 4 == sm and pitch >= n + ru.G
        for c in range(C):
            assert p[c] % 16 == 4 * ((want[c] + c * sm) % 4), (layout, c)
            assert r.view[c].ctypes.data == p[c] and r.view.shape == (C, n)
        # guards of at least G floats around every row, all of it SENTINEL
        lo = (np.array(p) - r.whole.ctypes.data) // 4
        assert lo[0] >= ru.G and np.all(np.diff(lo) >= n + ru.G) and r.whole.size - (lo[-1] + n) >= ru.G
        assert np.all(r.words() == ru.SENTINEL)
    assert {k: ru.offsets(v[0], 3) for k, v in ru.LAYOUTS.items()}["mixed"] == (0, 1, 2)
    assert ru.LAYOUTS["both2"][:2] == (2, 2) and ru.LAYOUTS["in3_out1"][:2] == (3, 1)


def test_numpy_and_strided_view_agree():
    r = ru.Rows(2, 10, (0, 1), 0)
    x = np.arange(20, dtype=np.float32).reshape(2, 10)
    r.fill(x, 7)
    got = r.numpy()
    assert np.array_equal(got[:, :7], x[:, :7]) and np.all(np.isnan(got[:, 7:]))
    assert np.all(got[:, 7:].view(np.int32) == ru.SENTINEL)


@pytest.mark.parametrize("layout", ru.ALL)
def test_correct_fake_kernel_passes(layout):
    x, xin, out = buffers(layout)
    fake_gain(xin.view, out.view, 1001, 1024)
    out.check_output()
    y = out.numpy()
    ru.assert_finite(y)
    assert np.array_equal(y[:, :1001], 2 * x) and not y[:, 1001:].any()


@pytest.mark.parametrize("layout", ["base", "out1", "mixed"])
def test_write_into_a_guard_is_caught(layout):
    _, xin, out = buffers(layout)
    fake_gain(xin.view, out.view, 1001, 1024, write=1025)   # one word past the row
    out.check_written()
    with pytest.raises(AssertionError, match="outside the rows"):
        out.check_guards()
    with pytest.raises(AssertionError):
        out.check_output()
    # ... and one word before a row
    _, xin, out = buffers(layout)
    fake_gain(xin.view, out.view, 1001, 1024)
    out.whole[out.starts[1] - 1] = 0.0
    with pytest.raises(AssertionError, match="outside the rows"):
        out.check_guards()


@pytest.mark.parametrize("layout", ["base", "out1", "mixed"])
def test_unwritten_word_is_caught(layout):
    _, xin, out = buffers(layout)
    fake_gain(xin.view, out.view, 1001, 1024, write=1023)   # the last word of every row left alone
    out.check_guards()
    with pytest.raises(AssertionError, match="never written"):
        out.check_written()
    with pytest.raises(AssertionError):
        out.check_output()


@pytest.mark.parametrize("layout", ["base", "in1", "mixed", "odd_stride"])
def test_read_past_L_is_caught(layout):
    _, xin, out = buffers(layout)
    fake_gain(xin.view, out.view, 1001, 1024, read=1002)    # consumes x[L]
    out.check_guards()   # (the NaN it produced may carry SENTINEL's own bits: check_written is not asked)
    with pytest.raises(AssertionError, match="non-finite"):
        ru.assert_finite(out.numpy())
    # the same with L told through a shorter length inside a longer row
    x, _, out = buffers(layout)
    io, _, sm = ru.LAYOUTS[layout]
    xin = ru.Rows(3, 1001, io, sm).fill(x, 900)
    fake_gain(xin.view, out.view, 900, 1024, read=901)
    with pytest.raises(AssertionError, match="non-finite"):
        ru.assert_finite(out.numpy())


def test_partial_rows_of_frames():
    """Magnitude rows: F frames of ld floats, K written; columns K..ld stay SENTINEL."""
    r = ru.Rows(2, 3 * 8, 1, 0)
    v = r.view.reshape(2, 3, 8) if r.view.flags["C_CONTIGUOUS"] else None
    assert v is None   # a strided view: index rows instead
    for c in range(2):
        np.lib.stride_tricks.as_strided(r.view[c], (3, 5), (32, 4))[:] = 1.0
    r.check_output(24, K=5, ld=8)
    r.view[1, 8 + 5] = 1.0   # column K of frame 1
    with pytest.raises(AssertionError, match="outside the rows"):
        r.check_output(24, K=5, ld=8)


def test_same_bits():
    a = np.array([0.0, 1.0], np.float32)
    assert ru.same_bits(a, a.copy()) and not ru.same_bits(a, np.array([-0.0, 1.0], np.float32))
