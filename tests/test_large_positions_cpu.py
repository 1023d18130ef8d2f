"""bigutil's closed forms against the oracle at small sizes (no GPU): what
test_gpu_large_positions.py expects at positions past 2^32 is the same
arithmetic in unbounded integers."""
import numpy as np
import pytest

import bigutil as bu

SR = 48000.0


def rnd(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)


def test_offsets_are_what_the_cases_need():
    """Every accepted offset is a multiple of B at or above 2^32 - 2B; the
    listed offsets stay as they are for power-of-two blocks; at B = 100 and
    384 a position truncated to 32 bits has another phase (so a kernel that
    narrows before `% B` renders another block phase), at B = 512 it has not."""
    for B in (512, 4096):
        assert bu.accepted_offsets(B) == bu.offsets(B)
        assert bu.refused_offsets(B) == list(bu.UNALIGNED)
    for B in (100, 384, 512, 4096):
        acc = bu.accepted_offsets(B)
        assert len(acc) == 5
        for (_, O), (_, A) in zip(bu.offsets(B), acc):
            assert A % B == 0 and 0 <= A - O < B
        assert acc[0][1] + B < bu.P32 < acc[0][1] + 3 * B  # crosses 2^32 in its third block
        assert all(O % B for O in bu.refused_offsets(B)) and len(bu.refused_offsets(B)) >= 2
    assert bu.P32 % 100 == 96 and bu.P32 % 384 == 256 and bu.P32 % 512 == 0
    for B in (100, 384):
        for _, O in bu.accepted_offsets(B)[1:]:
            assert bu.phase(O, B) == 0 and (O % bu.P32) % B != 0, (B, O)
    assert max(O for _, O in bu.offsets(4096)) + (1 << 24) < 1 << 63


@pytest.mark.parametrize("B", [512, 100, 384])
def test_ramp_slice_is_the_oracles_render_at_that_position(oracle, B):
    """IR_test restarts its ramp at every block: the oracle's render of a long
    file, from global sample O on, is ramp_slice of a short render."""
    plug = oracle.restated_plugin("IR_test")
    n = 3 * B + 17
    long_ = oracle.render_offline([], 2, B, SR, plug, L=40 * B)
    short = oracle.render_offline([], 2, B, SR, plug, L=n + B)
    for O in (0, B, 7 * B, 1, B - 1, 5 * B + 3, 20 * B + B // 2):
        assert np.array_equal(bu.ramp_slice(short, O, B, n), long_[:, O:O + n]), O
    tile = oracle.ir_ramp_reference(0.9, 0.002, B)
    assert np.array_equal(short[0, :2 * B], np.tile(tile, 2))


@pytest.mark.parametrize("name", ["gain_test", "static_gain_plugin", "no_op"])
def test_gain_kinds_do_not_depend_on_the_position(oracle, name):
    """The gain kinds are the same map at every position: the render of a
    slice is the slice of the render."""
    B = 100
    x = rnd((2, 30 * B), 1)
    plug = oracle.restated_plugin(name)
    whole = oracle.render_offline([x[0], x[1]], 2, B, SR, plug)
    for O in (0, 3 * B, 11 * B):
        part = oracle.render_offline([x[0, O:O + 5 * B], x[1, O:O + 5 * B]], 2, B, SR, plug)
        assert np.array_equal(part, whole[:, O:O + 5 * B])


@pytest.mark.parametrize("L,B,nblocks,cursor", [(1000, 512, 9, 997), (5000, 100, 120, 4999), (300, 384, 5, 123)])
def test_loop_index(oracle, L, B, nblocks, cursor):
    x = rnd((2, L), 2)
    ref, cur = oracle.render_loop([x[0], x[1]], 2, B, nblocks, SR, oracle.restated_plugin("no_op"), cursor=cursor)
    idx = bu.loop_index(cursor, 0, nblocks * B, L)
    assert np.array_equal(ref, x[:, idx])
    assert cur == (cursor + nblocks * B) % L
    mid = bu.loop_index(cursor, 700, 900, L)
    assert np.array_equal(mid, idx[700:900])


@pytest.mark.parametrize("n", [10_007, 12_345])
@pytest.mark.parametrize("P", [1920, 700, 19])
def test_minmax_closed_form(oracle, n, P):
    """The planted zero row: the closed form equals oracle.minmax_decimate."""
    vals = bu.planted(n, (P, 1920))
    assert len(vals) >= 12 and all(0 < abs(v) < 1 for v in vals.values())
    assert len(set(float(v) for v in vals.values())) == len(vals)
    x = np.zeros(n, np.float32)
    for s, v in vals.items():
        x[s] = v
    vmax, vmin = oracle.minmax_decimate(x, P)
    emax, emin = bu.minmax_expect(vals, n, P)
    assert np.array_equal(vmax, emax) and np.array_equal(vmin, emin)
    # the planted samples straddle pixel boundaries: neighbours land in different pixels
    s = bu.pixel_first(P // 3, P, n)
    assert bu.pixel_of(s - 1, P, n) == P // 3 - 1 and bu.pixel_of(s, P, n) == P // 3


def test_pixel_first_inverts_pixel_of():
    for n, P in ((1000, 192), (10_007, 1920), (97, 13)):
        for p in range(P):
            lo, hi = bu.pixel_first(p, P, n), bu.pixel_first(p + 1, P, n)
            assert all(bu.pixel_of(s, P, n) == p for s in range(lo, hi))
        assert bu.pixel_first(P, P, n) == n
    n = bu.P32 + 12_345
    for P in (1920, 70_000):
        for p in (1, P // 3, P - 1):
            s = bu.pixel_first(p, P, n)
            assert bu.pixel_of(s - 1, P, n) == p - 1 and bu.pixel_of(s, P, n) == p
        assert bu.pixel_first(P, P, n) == n
        # a 32-bit product would put these samples elsewhere
        assert any((p * n) % bu.P32 != p * n for p in (1, P // 3, P - 1))


def test_planted_positions_of_the_large_row():
    n = bu.P32 + 12_345
    vals = bu.planted(n, (1920, 70_000))
    for s in (0, bu.P31 - 1, bu.P31 + 1, bu.P32 - 1, bu.P32, bu.P32 + 1, n - 1):
        assert s in vals
    assert len(vals) == 7 + 24 and all(0 <= s < n for s in vals)


@pytest.mark.parametrize("F,P", [(1000, 192), (1234, 77)])
def test_spectrogram_bounds(oracle, F, P):
    """Pixel p of the spectrogram overview is the maximum over the frames
    [pixel_first(p), pixel_first(p + 1))."""
    mag = np.abs(rnd((F, 33), 3))
    ref = oracle.spectrogram_decimate(mag, P)
    for p in range(P):
        f0, f1 = bu.pixel_first(p, P, F), bu.pixel_first(p + 1, P, F)
        assert f1 > f0
        assert np.array_equal(ref[p], mag[f0:f1].max(axis=0)), p


def test_first_row_past_4gib():
    assert bu.first_row_past(bu.P32, 4097) == 262_081
    for ld in (4097, 4100, 513, 516):
        f = bu.first_row_past(bu.P32, ld)
        assert f * ld * 4 >= bu.P32 > (f - 1) * ld * 4
