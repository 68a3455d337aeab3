"""Numpy restatement of the angular intra costs, the best angular mode and the decision merge
(mip_angular_device) -- test helper, not a test.  Written from the contract text in
include/mipgpu.h alone: the boundaries and the corner by linear index, the angle and inverse
tables, the extended reference ref[k] with its projection and substitution, the 2-tap predictor,
PDPC of modes 18 and 50 with the explicit weight cut, SAD / SATD from predict_ref.sad_blocks /
satd_blocks.  Vectorised per shape: all CUs of a shape and all modes of the list at once.

tests/test_angular_cpu.py pins it by hand-checkable cases; the C++ host walk and the GPU kernel
are compared against it bit for bit.
"""
from __future__ import annotations

import numpy as np

import predict_ref as P
from mipgpu import layout

UNAVAILABLE = layout.UNAVAILABLE
FIRST, LAST, MODES = 2, 66, 65
MODE_BASE = 0x80
MAX_BIAS = 1 << 20
ALL_MODES = tuple(range(FIRST, LAST + 1))

_STEPS = (1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 23, 26, 29, 32)
ANGLE = dict(zip(range(2, 19), tuple(reversed(_STEPS)) + (0,)))
ANGLE.update(zip(range(19, 35), (-a for a in _STEPS)))
ANGLE.update(zip(range(35, 51), tuple(-a for a in reversed(_STEPS[:-1])) + (0,)))
ANGLE.update(zip(range(51, 67), _STEPS))
INVERSE = dict(zip(_STEPS, (16384, 8192, 5461, 4096, 2731, 2048, 1638, 1365, 1170, 1024, 910, 819, 712, 630, 565, 512)))


def _log2(v):
    v = int(v)
    assert v > 0 and v & (v - 1) == 0
    return v.bit_length() - 1


def _modes(modes):
    modes = ALL_MODES if modes is None else tuple(int(m) for m in modes)
    assert modes and all(FIRST <= m <= LAST for m in modes) and all(a < b for a, b in zip(modes, modes[1:])), modes
    return modes


def boundaries(refs, x, y, w, h):
    """(top [n, w], left [n, h], corner [n]) int64 of the w x h CUs at frame positions x, y [n]:
    the MIP path's complete boundaries and the corner, read by linear index."""
    flat = np.asarray(refs).reshape(-1).astype(np.int64)
    W = refs.shape[1]
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    last = flat.size - 1
    ti = (y[:, None] - 1) * W + x[:, None] + np.arange(w)[None, :]
    top = np.where(y[:, None] > 0, flat[np.clip(ti, 0, last)], np.where(x[:, None] > 0, flat[np.clip(x[:, None] - 1, 0, last)], 512))
    li = (y[:, None] + np.arange(h)[None, :]) * W + x[:, None] - 1
    left = np.where(x[:, None] > 0, flat[np.clip(li, 0, last)], np.where(y[:, None] > 0, flat[np.clip((y[:, None] - 1) * W, 0, last)], 512))
    corner = np.where((x > 0) & (y > 0), flat[np.clip((y - 1) * W + x - 1, 0, last)], top[:, 0])
    assert np.all(ti[y > 0] <= last) and np.all(li[x > 0] <= last)       # (only masked-out indexes were clipped)
    return top, left, corner


def weight(d, scale):
    """PDPC weight of the boundary sample at distance d."""
    s = (2 * np.asarray(d)) >> scale
    return np.where(s <= 5, 32 >> np.minimum(s, 5), 0)


def predict(top, left, corner, w, h, modes=None, pdpc=True, clip=True):
    """The predicted blocks, int64 [len(modes), n, h, w], of boundaries top [n, w], left [n, h],
    corner [n]; pdpc=False leaves the PDPC of modes 18 and 50 and the clip out (P of the
    contract); clip=False leaves only the clip out (the value the clip of the contract sees)."""
    modes = _modes(modes)
    top, left, corner = np.asarray(top, np.int64), np.asarray(left, np.int64), np.asarray(corner, np.int64)
    lw, lh = _log2(w), _log2(h)
    i, j = np.broadcast_to(np.arange(w)[None, :], (h, w)), np.broadcast_to(np.arange(h)[:, None], (h, w))
    out = np.empty((len(modes), top.shape[0], h, w), np.int64)
    for q, m in enumerate(modes):
        A = ANGLE[m]
        if m >= 34:
            main, side, a, b = top, left, i, j
        else:
            main, side, a, b = left, top, j, i
        M, S = main.shape[1], side.shape[1]
        # base[S - t] = side'[t] (t = 0..S, side'[0] = corner), base[S + u] = main[u - 1] (u = 1..M)
        base = np.concatenate([side[:, ::-1], corner[:, None], main], axis=1)
        inv = INVERSE[abs(A)] if A else 0

        def ref(k):
            t = np.minimum((-k * inv + 256) >> 9, S)
            pos = np.where(k >= 1, S + np.minimum(k, M), np.where(k == 0, S, S - t))
            assert A < 0 or np.all(k >= 1)
            return base[:, pos]

        d = (b + 1) * A
        idx, f = d >> 5, d & 31
        r0 = ref(a + idx + 1)
        p = np.where(f != 0, ((32 - f) * r0 + f * ref(a + idx + 2) + 16) >> 5, r0)
        if pdpc and m in (18, 50):
            scale = (lw + lh - 2) >> 2
            c = corner[:, None, None]
            if m == 50:
                wl, wt = weight(i, scale), 0
                ref_l, ref_t = left[:, :, None] - c + p, 0
            else:
                wl, wt = 0, weight(j, scale)
                ref_l, ref_t = 0, top[:, None, :] - c + p
            p = (ref_l * wl + ref_t * wt + (64 - wl - wt) * p + 32) >> 6
        out[q] = np.clip(p, 0, 1023) if pdpc and clip else p
    return out


def cu_costs(frame, refs, x, y, w, h, modes=None):
    """(sad, satd, cost), each [len(modes)], of ONE w x h CU at frame position (x, y)."""
    top, left, corner = boundaries(refs, [x], [y], w, h)
    orig = P.linear_block(frame, x, y, w, h)
    blocks = predict(top, left, corner, w, h, modes)[:, 0]
    sad, satd = P.sad_blocks(orig[None], blocks), P.satd_blocks(orig[None], blocks)
    return sad, satd, np.minimum(2 * sad, satd)


def tables(frame, refs, unavailable, modes=None):
    """dict of 'cost', 'sad', 'satd' int32 [nCTUs*5380, 65] for one frame [H, W], slot m - 2;
    `unavailable` bool [nCTUs*5380]: those CUs get UNAVAILABLE in every slot and read nothing;
    slots of modes not in `modes` (None: all 65) are UNAVAILABLE too."""
    modes = _modes(modes)
    height, width = frame.shape
    ncu = layout.num_ctus(width, height) * layout.CUS_PER_CTU
    unavailable = np.asarray(unavailable, bool)
    assert unavailable.shape == (ncu,)
    shape, x, y, _, _ = layout.cu_geometry(width, height, np.arange(ncu))
    sad = np.full((ncu, MODES), UNAVAILABLE, np.int64)
    satd = sad.copy()
    flat = np.asarray(frame).reshape(-1).astype(np.int64)
    slots = np.array(modes) - FIRST
    for s in layout.SHAPES:
        k = np.nonzero((shape == s.index) & ~unavailable)[0]
        if not k.size:
            continue
        top, left, corner = boundaries(refs, x[k], y[k], s.w, s.h)
        idx = (y[k, None, None] + np.arange(s.h)[None, :, None]).astype(np.int64) * width + x[k, None, None] + np.arange(s.w)[None, None, :]
        orig = flat[idx]
        blocks = predict(top, left, corner, s.w, s.h, modes)
        sad[k[:, None], slots[None, :]] = P.sad_blocks(orig[None], blocks).T
        satd[k[:, None], slots[None, :]] = P.satd_blocks(orig[None], blocks).T
    cost = np.where(sad == UNAVAILABLE, UNAVAILABLE, np.minimum(2 * sad, satd))
    return {"cost": cost.astype(np.int32), "sad": sad.astype(np.int32), "satd": satd.astype(np.int32)}


def best(cost):
    """(ang_mode uint8, ang_cost int32) [...] of cost tables [..., 65]: the lowest cost, ties to
    the lower mode, as MODE_BASE + m; 0xff / UNAVAILABLE where every slot is UNAVAILABLE."""
    cost = np.asarray(cost, np.int64)
    slot = cost.argmin(axis=-1)                                 # (the first of equal minima)
    low = np.take_along_axis(cost, slot[..., None], axis=-1)[..., 0]
    mode = np.where(low == UNAVAILABLE, 0xFF, MODE_BASE + FIRST + slot).astype(np.uint8)
    return mode, low.astype(np.int32)


def merge(best_mode, best_cost, ang_mode, ang_cost, bias=0):
    """The merge rule: the best angular mode replaces the current decision only if ang_cost + bias
    is strictly lower; CUs unavailable on either side stay.  Returns new (best_mode, best_cost)."""
    mode, cur = np.array(best_mode, np.uint8), np.array(best_cost, np.int64)
    ang_mode, ang_cost = np.broadcast_to(ang_mode, mode.shape), np.broadcast_to(np.asarray(ang_cost, np.int64), cur.shape)
    cand = ang_cost + int(bias)
    take = (cur != UNAVAILABLE) & (ang_cost != UNAVAILABLE) & (cand < cur)
    mode[take], cur[take] = ang_mode[take], cand[take]
    return mode, cur.astype(np.int32)
