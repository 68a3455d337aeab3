"""Numpy restatement of the Planar / DC baseline costs and the decision merge
(mip_intra_device) -- test helper, not a test.  Written from the contract text in
include/mipgpu.h alone: boundaries from predict_ref.boundaries (the oracle's
mipo_cu_boundaries), topRight / bottomLeft substituted by top[w-1] / left[h-1], Planar, DC, PDPC
with the explicit weight cut, SAD / SATD from predict_ref.sad_blocks / satd_blocks.  Vectorised
per shape: all CUs of a shape are predicted at once.

tests/test_intra_cpu.py pins it by hand-checkable cases; the C++ host walk and the GPU kernel
are compared against it bit for bit.
"""
from __future__ import annotations

import numpy as np

import predict_ref as P
from mipgpu import layout

UNAVAILABLE = layout.UNAVAILABLE
MODE_PLANAR, MODE_DC = 0xF0, 0xF1
MAX_BIAS = 1 << 20


def _log2(v):
    assert v > 0 and v & (v - 1) == 0
    return v.bit_length() - 1


def predict(top, left, w, h):
    """Planar and DC blocks after PDPC for boundaries top [n, w], left [n, h]:
    (planar, dc), each int64 [n, h, w]."""
    top, left = np.asarray(top, np.int64), np.asarray(left, np.int64)
    lw, lh = _log2(w), _log2(h)
    i, j = np.arange(w)[None, None, :], np.arange(h)[None, :, None]
    t, l = top[:, None, :], left[:, :, None]
    tr, bl = top[:, w - 1][:, None, None], left[:, h - 1][:, None, None]
    pred_v = ((h - 1 - j) * t + (j + 1) * bl) << lw
    pred_h = ((w - 1 - i) * l + (i + 1) * tr) << lh
    planar = (pred_v + pred_h + w * h) >> (lw + lh + 1)
    st, sl = top.sum(axis=1), left.sum(axis=1)
    if w == h:
        dc = (st + sl + w) >> (lw + 1)
    elif w > h:
        dc = (st + (w >> 1)) >> lw
    else:
        dc = (sl + (h >> 1)) >> lh
    dc = np.broadcast_to(dc[:, None, None], planar.shape)
    scale = (lw + lh - 2) >> 2
    s_t, s_l = (2 * j) >> scale, (2 * i) >> scale
    w_t = np.where(s_t <= 5, 32 >> np.minimum(s_t, 5), 0)
    w_l = np.where(s_l <= 5, 32 >> np.minimum(s_l, 5), 0)

    def pdpc(p):
        return np.clip((l * w_l + t * w_t + (64 - w_l - w_t) * p + 32) >> 6, 0, 1023)

    return pdpc(planar), pdpc(dc)


def cu_costs(frame, refs, x, y, w, h):
    """(sad[2], satd[2], cost[2]) of ONE w x h CU at frame position (x, y) -- any power-of-two
    size, also ones that are not among the 47 shapes."""
    top, left, _, _ = P.boundaries(refs, x, y, w, h)
    orig = P.linear_block(frame, x, y, w, h)
    blocks = np.stack([b[0] for b in predict(top[None], left[None], w, h)])
    sad, satd = P.sad_blocks(orig[None], blocks), P.satd_blocks(orig[None], blocks)
    return sad, satd, np.minimum(2 * sad, satd)


def tables(frame, refs, unavailable):
    """dict of 'cost', 'sad', 'satd' int32 [nCTUs*5380, 2] for one frame [H, W]; `unavailable`
    bool [nCTUs*5380] (mipgpu.unavailable_cus of the reference source): those CUs get
    UNAVAILABLE in all three and read nothing."""
    height, width = frame.shape
    ncu = layout.num_ctus(width, height) * layout.CUS_PER_CTU
    unavailable = np.asarray(unavailable, bool)
    assert unavailable.shape == (ncu,)
    shape, x, y, bw, bh = layout.cu_geometry(width, height, np.arange(ncu))
    sad = np.full((ncu, 2), UNAVAILABLE, np.int64)
    satd = sad.copy()
    flat = np.asarray(frame).reshape(-1)
    for s in layout.SHAPES:
        k = np.nonzero((shape == s.index) & ~unavailable)[0]
        if not k.size:
            continue
        b = [P.boundaries(refs, x[c], y[c], s.w, s.h)[:2] for c in k]
        top, left = np.stack([t for t, _ in b]), np.stack([l for _, l in b])
        idx = (y[k, None, None] + np.arange(s.h)[None, :, None]).astype(np.int64) * width + x[k, None, None] + np.arange(s.w)[None, None, :]
        orig = flat[idx]
        for m, blk in enumerate(predict(top, left, s.w, s.h)):
            sad[k, m] = P.sad_blocks(orig, blk)
            satd[k, m] = P.satd_blocks(orig, blk)
    cost = np.where(sad == UNAVAILABLE, UNAVAILABLE, np.minimum(2 * sad, satd))
    return {"cost": cost.astype(np.int32), "sad": sad.astype(np.int32), "satd": satd.astype(np.int32)}


def merge(best_mode, best_cost, cost, bias=None):
    """The merge rule: candidates MIP, Planar, DC, a later one replaces the current one only if
    cost + bias is strictly lower; unavailable CUs stay.  Returns new (best_mode, best_cost)."""
    bias = (0, 0) if bias is None else bias
    mode, cur = np.array(best_mode, np.uint8), np.array(best_cost, np.int64)
    cost = np.asarray(cost, np.int64).reshape(cur.shape + (2,))
    for m, code in ((0, MODE_PLANAR), (1, MODE_DC)):
        cand = cost[..., m] + int(bias[m])
        take = (cur != UNAVAILABLE) & (cost[..., m] != UNAVAILABLE) & (cand < cur)
        mode[take], cur[take] = code, cand[take]
    return mode, cur.astype(np.int32)
