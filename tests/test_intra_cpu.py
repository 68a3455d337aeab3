"""Hand-checkable pins of the numpy restatement of the Planar / DC baseline costs
(tests/intra_ref.py, written from the contract in include/mipgpu.h), and the Python constants
that go with mip_intra_device.  No GPU."""
import numpy as np
import pytest

import intra_ref as I
import mipgpu
from mipgpu import layout


def test_uniform_frame_costs_nothing_inside_and_512_at_the_origin():
    w, h, v = 136, 72, 700
    frame = np.full((h, w), v, np.uint16)
    un = mipgpu.unavailable_cus(w, h)
    t = I.tables(frame, frame, un)
    _, x, y, bw, bh = layout.cu_geometry(w, h, np.arange(un.size))
    inside = ~un & (x > 0) & (y > 0)
    assert inside.any() and np.all(t["cost"][inside] == 0) and np.all(t["sad"][inside] == 0) and np.all(t["satd"][inside] == 0)
    origin = np.nonzero(~un & (x == 0) & (y == 0))[0]
    assert origin.size > 1 and origin[0] == 0                 # the first 64x64 CU among them
    # all boundaries are 512: Planar, DC and PDPC of a constant are the constant
    assert np.array_equal(t["sad"][origin], np.repeat((bw[origin] * bh[origin] * abs(v - 512))[:, None], 2, axis=1))
    assert np.all(t["cost"][un] == layout.UNAVAILABLE) and np.all(t["sad"][un] == layout.UNAVAILABLE)


@pytest.mark.parametrize("size", ((4, 64), (64, 4)), ids=("4x64", "64x4"))
def test_weight_cut_of_long_blocks(size):
    """scale = (2 + 6 - 2) >> 2 = 1: the shift (2*d) >> 1 = d passes 5 at the sixth row / column,
    where the boundary weight is exactly 0 (not 32 >> d, which wraps for d >= 32)."""
    w, h = size
    top, left = np.full((1, w), 1000), np.full((1, h), 0)
    planar, dc = I.predict(top, left, w, h)
    want_dc = (1000 * w + (w >> 1)) >> (w.bit_length() - 1) if w > h else (0 + (h >> 1)) >> (h.bit_length() - 1)
    long_axis = np.arange(max(w, h))
    wt = np.where(long_axis <= 5, 32 >> np.minimum(long_axis, 5), 0)
    short = np.arange(4)
    ws = 32 >> short                                          # shifts 0..3 on the short side
    if h > w:   # rows are the long axis: wT = wt[j], wL = ws[i]
        want = (0 * ws[None, :] + 1000 * wt[:, None] + (64 - ws[None, :] - wt[:, None]) * want_dc + 32) >> 6
    else:
        want = (0 * wt[None, :] + 1000 * ws[:, None] + (64 - wt[None, :] - ws[:, None]) * want_dc + 32) >> 6
    assert np.array_equal(dc[0], np.clip(want, 0, 1023))
    assert planar.min() >= 0 and planar.max() <= 1023
    # row / column 40 sees no top / left boundary at all
    if h > w:
        assert np.array_equal(dc[0, 40], (0 * ws + (64 - ws) * want_dc + 32) >> 6)
    else:
        assert np.array_equal(dc[0, :, 40], (1000 * ws + (64 - ws) * want_dc + 32) >> 6)


def test_dc_rule_by_aspect():
    """Top boundary 800, left boundary 200, no PDPC reach at the far corner: the DC value is the
    top mean (w > h), the left mean (h > w) or the mean of both (w == h)."""
    for w, h, want in ((32, 8, 800), (8, 32, 200), (16, 16, 500), (32, 32, 500)):
        _, dc = I.predict(np.full((1, w), 800), np.full((1, h), 200), w, h)
        assert dc[0, h - 1, w - 1] == want, (w, h)
    # rounding: sums that are not multiples of the divisor
    _, dc = I.predict(np.array([[1, 2, 3, 5, 0, 0, 0, 0]]), np.array([[9, 9, 9, 9]]), 8, 4)
    assert dc[0, 3, 7] == (11 + 4) >> 3
    _, dc = I.predict(np.array([[1, 2, 3, 5]]), np.array([[9, 9, 9, 8]]), 4, 4)
    assert dc[0, 3, 3] == (11 + 35 + 4) >> 3


def test_planar_by_hand():
    """4x4, top = left = (0, 0, 0, 64): topRight = bottomLeft = 64; sample (3, 3) has
    predV = (0*64 + 4*64) << 2, predH the same, P = (2048 + 16) >> 5 = 64, and no PDPC weight
    beyond shift 6 (scale 0: shift 2*3 = 6 > 5)."""
    b = np.array([[0, 0, 0, 64]])
    planar, _ = I.predict(b, b, 4, 4)
    assert planar[0, 3, 3] == 64
    # sample (0, 0): predV = (3*0 + 1*64) << 2 = 256 = predH, P = (512 + 16) >> 5 = 16; wT = wL = 32: (0 + 0 + 0*16 + 32) >> 6
    assert planar[0, 0, 0] == 0


def test_one_cu_on_a_frame_whose_boundaries_differ():
    w, h = 64, 64
    frame = np.zeros((h, w), np.uint16)
    frame[15, :] = 800                                        # the row above y = 16
    frame[:, 15] = 200                                        # the column left of x = 16
    for bw, bh, want in ((32, 8, 800), (8, 32, 200), (16, 16, 500)):
        sad, satd, cost = I.cu_costs(frame, frame, 16, 16, bw, bh)
        top, left, _, _ = I.P.boundaries(frame, 16, 16, bw, bh)
        assert np.all(top == 800) and np.all(left == 200)
        _, dc = I.predict(top[None], left[None], bw, bh)
        assert dc[0, bh - 1, bw - 1] == want
        assert sad[1] == dc[0].sum() and cost[1] == min(2 * sad[1], satd[1])   # originals are 0 inside


def test_merge_rule():
    un = layout.UNAVAILABLE
    mode = np.array([3, 3, 3, 3, 0xFF, 3], np.uint8)
    cost = np.array([100, 100, 100, 100, un, 100], np.int32)
    tab = np.array([[100, 100], [99, 99], [99, 98], [101, 100], [5, 5], [un, un]], np.int32)
    m, c = I.merge(mode, cost, tab)
    assert m.tolist() == [3, I.MODE_PLANAR, I.MODE_DC, 3, 0xFF, 3] and c.tolist() == [100, 99, 98, 100, un, 100]
    m, c = I.merge(mode, cost, tab, (1 << 20, 1))
    assert m.tolist() == [3, 3, I.MODE_DC, 3, 0xFF, 3] and c.tolist() == [100, 100, 99, 100, un, 100]


def test_python_constants():
    assert mipgpu.MODE_PLANAR == I.MODE_PLANAR == 0xF0 and mipgpu.MODE_DC == I.MODE_DC == 0xF1
    assert min(mipgpu.MODE_PLANAR, mipgpu.MODE_DC) >= max(s.total_modes for s in layout.SHAPES)
    assert mipgpu.INTRA_MAX_BIAS == I.MAX_BIAS
    assert mipgpu._bias(None) is None and mipgpu._bias((1, 2)).tolist() == [1, 2] and mipgpu._bias((1, 2)).dtype == np.int32
    for bad in ((1,), (1, 2, 3), (1 << 40, 0)):
        with pytest.raises(mipgpu.MipError):
            mipgpu._bias(bad)
