"""Numpy restatement of the angular family with extended reference lines (mip_angular_refs,
MIP_ANG_REFS_EXTENDED) -- test helper, not a test.  Written from the contract text in
include/mipgpu.h alone: the order key (CTU raster index, then the Morton code of the 4x4 block
inside the CTU, x in the even bits), the two lengths E_top / E_left per CU, and the predictor with
the main line of length M' = M + E(main).  The predictor itself is tests/angular_ref.py's, called
once per class with that class's main line made longer: past M' the line repeats its last sample,
which is what ref[k] = main[min(k, M') - 1] reads.

tests/test_angular_ext_cpu.py pins it by hand-checkable cases; mip_extended_refs, the C++ host
walks and the GPU kernels are compared against it bit for bit.
"""
from __future__ import annotations

import numpy as np

import angular_ref as A
import predict_ref as P
from mipgpu import layout

UNAVAILABLE = A.UNAVAILABLE
SUBSTITUTED, EXTENDED = 0, 1
POSITIVE_MODES = tuple(range(2, 18)) + tuple(range(51, 67))     # the modes with A > 0


def order_key(sx, sy, width):
    """The key of the sample at frame position (sx, sy) as one number: the pair (CTU raster index,
    Morton code < 1024) compared lexicographically."""
    sx, sy = np.asarray(sx, np.int64), np.asarray(sy, np.int64)
    cols = (width + 127) // 128
    bx, by = (sx % 128) >> 2, (sy % 128) >> 2
    morton = np.zeros_like(bx)
    for k in range(5):
        morton |= ((bx >> k) & 1) << (2 * k) | ((by >> k) & 1) << (2 * k + 1)
    return ((sy >> 7) * cols + (sx >> 7)) * 1024 + morton


def usable(width, height, unavailable, undefined=None):
    """(top, left) bool [nCTUs*5380, 64]: column n says whether the sample t = w + n of the top
    line (t = h + n of the left line) meets every condition of the rule, n < h (n < w), for a CU
    that is available and wholly inside the frame; all False for any other CU."""
    ncu = layout.num_ctus(width, height) * layout.CUS_PER_CTU
    unavailable = np.asarray(unavailable, bool)
    assert unavailable.shape == (ncu,)
    _, x, y, w, h = (np.asarray(v, np.int64)[:, None] for v in layout.cu_geometry(width, height, np.arange(ncu)))
    und = np.zeros(width * height, bool) if undefined is None else np.asarray(undefined, bool).reshape(-1)
    inside = ~unavailable[:, None] & (x + w <= width) & (y + h <= height)
    own = order_key(x, y, width)
    last = width * height - 1
    n = np.arange(64)[None, :]
    sx, sy = x + w + n, y - 1 + 0 * n
    top = inside & (n < h) & (y > 0) & (sx < width) & (order_key(np.minimum(sx, width - 1), np.maximum(sy, 0), width) < own) & \
        ~und[np.clip(sy * width + sx, 0, last)]
    sx, sy = x - 1 + 0 * n, y + h + n
    left = inside & (n < w) & (x > 0) & (sy < height) & (order_key(np.maximum(sx, 0), np.minimum(sy, height - 1), width) < own) & \
        ~und[np.clip(sy * width + sx, 0, last)]
    return top, left


def lengths(width, height, unavailable, undefined=None):
    """(E_top, E_left) int64 [nCTUs*5380]: the largest n such that every sample before n is usable.
    `unavailable` bool per CU (the availability set the lengths go with), `undefined` bool [H, W]
    or None: the reference samples an engine filter leaves undefined."""
    top, left = usable(width, height, unavailable, undefined)
    return np.cumprod(top, axis=1).sum(axis=1), np.cumprod(left, axis=1).sum(axis=1)


def boundaries(refs, x, y, w, h, e_top, e_left):
    """(top [n, w + h], left [n, h + w], corner [n]): angular_ref.boundaries' lines followed by
    their extensions -- top[t] = R[(y-1)*W + x + t] for t < w + E_top, left[t] = R[(y+t)*W + x - 1]
    for t < h + E_left -- and past those the last sample of each line again."""
    top, left, corner = A.boundaries(refs, x, y, w, h)
    flat = np.asarray(refs).reshape(-1).astype(np.int64)
    W = refs.shape[1]
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    e_top, e_left = np.asarray(e_top, np.int64), np.asarray(e_left, np.int64)
    last = flat.size - 1
    t = np.minimum(w + np.arange(h)[None, :], (w + e_top - 1)[:, None])            # [n, h], >= w - 1
    more = flat[np.clip((y[:, None] - 1) * W + x[:, None] + t, 0, last)]
    top = np.concatenate([top, np.where(e_top[:, None] > 0, more, top[:, -1:])], axis=1)
    t = np.minimum(h + np.arange(w)[None, :], (h + e_left - 1)[:, None])
    more = flat[np.clip((y[:, None] + t) * W + x[:, None] - 1, 0, last)]
    left = np.concatenate([left, np.where(e_left[:, None] > 0, more, left[:, -1:])], axis=1)
    return top, left, corner


def predict(top, left, corner, w, h, modes=None):
    """The predicted blocks, int64 [len(modes), n, h, w], of boundaries() lines: the vertical class
    with the long top line as its main line and left[0..h) as its side, the horizontal class with
    the long left line and top[0..w)."""
    modes = A._modes(modes)
    out = np.empty((len(modes), top.shape[0], h, w), np.int64)
    vert = [q for q, m in enumerate(modes) if m >= 34]
    hor = [q for q, m in enumerate(modes) if m < 34]
    if vert:
        out[vert] = A.predict(top, left[:, :h], corner, w, h, [modes[q] for q in vert])
    if hor:
        out[hor] = A.predict(top[:, :w], left, corner, w, h, [modes[q] for q in hor])
    return out


def tables(frame, refs, unavailable, e_top, e_left, modes=None):
    """angular_ref.tables with the lengths e_top / e_left [nCTUs*5380] of the same set."""
    modes = A._modes(modes)
    height, width = frame.shape
    ncu = layout.num_ctus(width, height) * layout.CUS_PER_CTU
    unavailable = np.asarray(unavailable, bool)
    assert unavailable.shape == (ncu,)
    shape, x, y, _, _ = layout.cu_geometry(width, height, np.arange(ncu))
    sad = np.full((ncu, A.MODES), UNAVAILABLE, np.int64)
    satd = sad.copy()
    flat = np.asarray(frame).reshape(-1).astype(np.int64)
    slots = np.array(modes) - A.FIRST
    for s in layout.SHAPES:
        k = np.nonzero((shape == s.index) & ~unavailable)[0]
        if not k.size:
            continue
        top, left, corner = boundaries(refs, x[k], y[k], s.w, s.h, e_top[k], e_left[k])
        idx = (y[k, None, None] + np.arange(s.h)[None, :, None]).astype(np.int64) * width + x[k, None, None] + np.arange(s.w)[None, None, :]
        orig = flat[idx]
        blocks = predict(top, left, corner, s.w, s.h, modes)
        sad[k[:, None], slots[None, :]] = P.sad_blocks(orig[None], blocks).T
        satd[k[:, None], slots[None, :]] = P.satd_blocks(orig[None], blocks).T
    cost = np.where(sad == UNAVAILABLE, UNAVAILABLE, np.minimum(2 * sad, satd))
    return {"cost": cost.astype(np.int32), "sad": sad.astype(np.int32), "satd": satd.astype(np.int32)}


def predict_cu(refs, x, y, w, h, e_top, e_left, mode):
    """The block [h, w] uint16 of ONE CU and one mode number."""
    top, left, corner = boundaries(refs, [x], [y], w, h, [e_top], [e_left])
    return predict(top, left, corner, w, h, (mode,))[0, 0].astype(np.uint16)
