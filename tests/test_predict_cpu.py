"""Prediction output, host side (no GPU): mip_pred_layout, the argument checks that run before
any HIP call, and the numpy restatement of a CU's prediction (tests/predict_ref.py) pinned to
the oracle's SAD / SATD tables -- which the golden fixtures pin to the reference's kernels."""
import ctypes

import numpy as np
import pytest

import mipgpu
import oracle_lib as O
import predict_ref as P
from mipgpu import layout
from mipgpu.synth import synth_frame

W, H = 136, 72          # two CTUs; CUs right of the frame wrap, CUs below it are unavailable
FILTER = "filterFrame_1d_int"


def _mixed_list(rng, n_per_shape=3):
    """A list over all 47 shapes and both CTUs, with mode-none and unavailable items."""
    prefix = np.cumsum([0] + [s.ncu for s in layout.SHAPES])
    cu, mode = [], []
    for s in layout.SHAPES:
        for ctu in range(layout.num_ctus(W, H)):
            for c in rng.integers(0, s.ncu, n_per_shape):
                cu.append(ctu * layout.CUS_PER_CTU + prefix[s.index] + int(c))
                mode.append(int(rng.integers(0, s.total_modes)))
    cu, mode = np.array(cu), np.array(mode)
    mode[::7] = 0xFF
    order = rng.permutation(cu.size)
    return cu[order], mode[order]


def test_packed_layout_is_the_prefix_sum_of_block_sizes():
    rng = np.random.default_rng(7)
    cu, mode = _mixed_list(rng)
    frame = rng.integers(0, 3, cu.size)
    items, total = mipgpu.pred_items(W, H, frame, cu, mode, layout="packed", nframes=3)
    assert items.dtype == mipgpu.PRED_ITEM and items.dtype.itemsize == 24
    shape, x, y, w, h = layout.cu_geometry(W, H, cu)
    assert set(shape) == set(range(47))
    un = mipgpu.unavailable_cus(W, H)
    assert un[cu].any() and (~un[cu]).any() and (mode == 0xFF).any()   # they reserve their block too
    sizes = w.astype(np.int64) * h
    assert np.array_equal(items["offset"], np.concatenate([[0], np.cumsum(sizes)[:-1]]))
    assert np.array_equal(items["pitch"], w)
    assert total == sizes.sum()
    assert np.array_equal(items["cu"], cu) and np.array_equal(items["mode"], mode) and np.array_equal(items["frame"], frame)


def test_frame_layout_is_the_linear_address():
    rng = np.random.default_rng(8)
    cu, mode = _mixed_list(rng)
    frame = rng.integers(0, 4, cu.size)
    items, total = mipgpu.pred_items(W, H, frame, cu, mode, layout="frame", nframes=4)
    _, x, y, _, _ = layout.cu_geometry(W, H, cu)
    assert np.array_equal(items["offset"], frame.astype(np.int64) * W * H + y.astype(np.int64) * W + x)
    assert np.all(items["pitch"] == W)
    assert total == 4 * W * H
    assert np.all(items["offset"] % 4 == 0)


def test_cu_geometry_matches_the_library():
    lib = mipgpu.library()
    prefix = np.cumsum([0] + [s.ncu for s in layout.SHAPES])
    for s in layout.SHAPES:
        for c in (0, s.ncu // 3, s.ncu - 1):
            shape, x, y, w, h = layout.cu_geometry(W, H, [layout.CUS_PER_CTU + prefix[s.index] + c])
            cx, cy = ctypes.c_int(), ctypes.c_int()
            assert lib.mip_cu_position(s.index, c, ctypes.byref(cx), ctypes.byref(cy)) == 0
            assert (shape[0], x[0], y[0], w[0], h[0]) == (s.index, 128 + cx.value, cy.value, s.w, s.h)
    with pytest.raises(ValueError):
        layout.cu_geometry(W, H, [2 * layout.CUS_PER_CTU])


@pytest.mark.parametrize("frame, cu, word", [(0, 2 * 5380, "cu"), (0, -1, "cu"), (2, 0, "frame"), (-1, 0, "frame")])
def test_layout_refuses_names_out_of_range(frame, cu, word):
    for lay in ("packed", "frame"):
        with pytest.raises(mipgpu.MipError, match=word):
            mipgpu.pred_items(W, H, [0, frame], [5, cu], [0, 0], layout=lay, nframes=2)
    with pytest.raises(mipgpu.MipError, match="layout"):
        mipgpu.pred_items(W, H, [0], [0], [0], layout="tiled")


def test_predict_frames_without_an_engine_fails_before_any_hip_call():
    lib = mipgpu.library()
    assert lib.mip_abi_version() == 7
    items, total = mipgpu.pred_items(W, H, [0], [0], [0])
    out = np.zeros(total, np.uint16)
    frame = np.zeros((1, H, W), np.uint16)
    skipped = ctypes.c_int64(-5)
    rc = lib.mip_predict_frames(None, frame.ctypes.data, None, 1, items.ctypes.data, 1, out.ctypes.data, total,
                                ctypes.byref(skipped))
    assert rc != 0 and b"engine is NULL" in lib.mip_last_error()
    assert lib.mip_predict_device(None, None, None, 1, None, 0, None, 0, None, None) != 0
    assert b"engine is NULL" in lib.mip_last_error()
    assert not out.any() and skipped.value == -5


def test_restatement_matches_the_oracle_tables():
    """SAD and SATD of every restated block against the originals (read at linear indexes) are
    the oracle's table entries: all modes of the sampled CUs of both CTUs, references from the
    separable 3-tap filter, whose last columns exceed 10 bits at this width."""
    frame = synth_frame(W, H, 0x51, 1)
    refs = O.filter_frame(frame, FILTER, 0)
    _, sad, satd = O.search(frame, refs, want_sad_satd=True)
    cus = P.sample_cus(W, H, mipgpu.unavailable_cus(W, H, FILTER))
    shape, x, y, w, h = layout.cu_geometry(W, H, cus)
    assert set(shape) == set(range(47))
    above, items = 0, 0
    for i, cu in enumerate(cus):
        s = layout.SHAPES[shape[i]]
        cp = P.CuPredictor(refs, x[i], y[i], s.index)
        above += cp.max_boundary > 1023
        orig = P.linear_block(frame, x[i], y[i], s.w, s.h)
        pred = np.stack([cp.predict(m) for m in range(s.total_modes)])
        base = (cu // layout.CUS_PER_CTU) * layout.COSTS_PER_CTU + s.cost_offset + \
            (cu % layout.CUS_PER_CTU - sum(t.ncu for t in layout.SHAPES[:s.index])) * s.total_modes
        assert np.array_equal(P.sad_blocks(orig[None], pred), sad[base:base + s.total_modes]), (cu, s.name)
        assert np.array_equal(P.satd_blocks(orig[None], pred), satd[base:base + s.total_modes]), (cu, s.name)
        items += s.total_modes
    assert items > 4000
    assert above > 0     # boundary samples above 1023 are covered (column 135 of the filtered frame)
    assert refs.max() > 1023
