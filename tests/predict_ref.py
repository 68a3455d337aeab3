"""Numpy restatement of one CU's MIP prediction -- test helper, not a test.

Boundaries and the reduced prediction come from the oracle's exported stage helpers
(mipo_cu_boundaries, mipo_reduced_pred; their argtypes are set here, oracle_lib.py is left
alone).  The upsampler is a vectorised restatement of the rules in oracle/mip_oracle.c's
comments (intra.cl:815-912): the horizontal pass runs on the anchor rows k*upV + upV-1 with the
left boundary as the first "before" sample, the vertical pass follows with the top boundary as
"before"; a factor of 1 is a copy; size_id 0 has no upsampling.

tests/test_predict_cpu.py pins this restatement to the oracle's SAD / SATD tables; the GPU
tests compare the engine's emitted blocks against it bit for bit.
"""
from __future__ import annotations

import ctypes

import numpy as np

import oracle_lib as O
from mipgpu import layout

_ready = False


def _lib():
    global _ready
    L = O.lib()
    if not _ready:
        u16p = np.ctypeslib.ndpointer(np.uint16, flags="C_CONTIGUOUS")
        i16p = np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS")
        ci = ctypes.c_int
        L.mipo_cu_boundaries.argtypes = [u16p, ci, ci, ci, ci, ci, ci, i16p, i16p, i16p, i16p]
        L.mipo_cu_boundaries.restype = None
        L.mipo_reduced_pred.argtypes = [ci, ci, ci, i16p, i16p, i16p]
        L.mipo_reduced_pred.restype = None
        _ready = True
    return L


def boundaries(refs, x, y, w, h):
    """(top[w], left[h], red_top[4], red_left[4]) of the CU at frame position (x, y), int16."""
    refs = np.ascontiguousarray(refs, np.uint16)
    top, left = np.zeros(w, np.int16), np.zeros(h, np.int16)
    rt, rl = np.zeros(4, np.int16), np.zeros(4, np.int16)
    _lib().mipo_cu_boundaries(refs, refs.shape[1], refs.shape[0], int(x), int(y), int(w), int(h), top, left, rt, rl)
    return top, left, rt, rl


def upsample(red, r, w, h, top, left):
    """Reduced prediction red[r, r] -> block [h, w] (int64)."""
    red = np.asarray(red, np.int64).reshape(r, r)
    top, left = np.asarray(top, np.int64), np.asarray(left, np.int64)
    uh, uv = w // r, h // r
    rows = np.arange(r) * uv + uv - 1                       # anchor rows
    if uh == 1:
        anchor = red.copy()
    else:
        lh = uh.bit_length() - 1
        before = np.concatenate([left[rows][:, None], red[:, :-1]], axis=1)   # [r, r]
        o = np.arange(1, uh + 1)                            # offset inside a window
        win = ((uh - o)[None, None, :] * before[:, :, None] + o[None, None, :] * red[:, :, None] + (1 << (lh - 1))) >> lh
        anchor = win.reshape(r, w)
    if uv == 1:
        return anchor
    lv = uv.bit_length() - 1
    before = np.concatenate([top[None, :], anchor[:-1]], axis=0)              # [r, w]
    o = np.arange(1, uv + 1)
    out = ((uv - o)[None, :, None] * before[:, None, :] + o[None, :, None] * anchor[:, None, :] + (1 << (lv - 1))) >> lv
    out = out.reshape(h, w)
    out[rows] = anchor                                      # anchor rows keep their values
    return out


class CuPredictor:
    """All modes of one CU: boundaries once, then predict(mode) -> uint16 [h, w]."""

    def __init__(self, refs, x, y, shape):
        s = layout.SHAPES[int(shape)]
        self.s, self.x, self.y = s, int(x), int(y)
        self.top, self.left, self.rt, self.rl = boundaries(refs, x, y, s.w, s.h)
        self.r = 8 if s.size_id == 2 else 4
        self.max_boundary = int(max(self.top.max(), self.left.max()))

    def predict(self, mode):
        s, r = self.s, self.r
        red = np.zeros(r * r, np.int16)
        _lib().mipo_reduced_pred(s.size_id, int(mode) % s.modes, int(int(mode) >= s.modes), self.rt, self.rl, red)
        if s.size_id == 0:
            return red.reshape(4, 4).astype(np.uint16)
        return upsample(red, r, s.w, s.h, self.top, self.left).astype(np.uint16)


def predict_cu(refs, width, height, cu, mode):
    """Predicted block (uint16 [h, w]) of CU index `cu` (decision-list order) at `mode`."""
    shape, x, y, _, _ = layout.cu_geometry(width, height, [cu])
    return CuPredictor(refs, x[0], y[0], shape[0]).predict(mode)


def linear_block(frame, x, y, w, h):
    """The w x h samples at (x, y) read by linear index y' * W + x' like the reference does
    (CUs right of the frame read the next row's samples)."""
    flat = np.asarray(frame).reshape(-1)
    W = frame.shape[1]
    idx = (y + np.arange(h))[:, None] * W + x + np.arange(w)[None, :]
    return flat[idx]


def sad_blocks(orig, pred):
    """SAD of blocks [..., h, w] (int64)."""
    return np.abs(np.asarray(orig, np.int64) - np.asarray(pred, np.int64)).sum(axis=(-1, -2))


def satd_blocks(orig, pred):
    """Sum of the 4x4 Hadamard SATDs of blocks [..., h, w], built as satd4x4 of
    oracle/mip_oracle.c (kernel_aux_functions.cl:142-249: DC term scaled by 1/4, (satd + 1) >> 1
    per 4x4 block)."""
    d = np.asarray(orig, np.int64) - np.asarray(pred, np.int64)
    h, w = d.shape[-2:]
    lead = d.shape[:-2]
    d = d.reshape(lead + (h // 4, 4, w // 4, 4))
    d = np.moveaxis(d, -3, -2)                              # [..., by, bx, 4 rows, 4 cols]
    r0, r1, r2, r3 = (d[..., i, :] for i in range(4))
    m0, m1, m2, m3 = r0 + r3, r1 + r2, r1 - r2, r0 - r3    # vertical butterflies
    e = np.stack([m0 + m1, m2 + m3, m0 - m1, m3 - m2], axis=-2)
    q0, q1, q2, q3 = (e[..., i] for i in range(4))
    t0, t1, t2, t3 = q0 + q3, q1 + q2, q1 - q2, q0 - q3    # horizontal butterflies
    m = np.abs(np.stack([t0 + t1, t0 - t1, t2 + t3, t3 - t2], axis=-1))   # [..., by, bx, 4, 4]
    s = m.sum(axis=(-1, -2))
    dc = m[..., 0, 0]
    s = s - dc + (dc >> 2)
    return ((s + 1) >> 1).sum(axis=(-1, -2))


def sample_cus(width, height, unavailable, seed=0x51, per_shape=6):
    """The CU sample of the prediction tests: for every shape and every CTU the first CU, the
    last CU and `per_shape` seeded random CUs, without the unavailable ones.  Sorted CU indexes."""
    rng = np.random.default_rng(seed)
    prefix = np.cumsum([0] + [s.ncu for s in layout.SHAPES])
    picked = []
    for ctu in range(layout.num_ctus(width, height)):
        for s in layout.SHAPES:
            local = {0, s.ncu - 1} | set(int(v) for v in rng.integers(0, s.ncu, per_shape))
            picked += [ctu * layout.CUS_PER_CTU + int(prefix[s.index]) + c for c in sorted(local)]
    picked = np.array(sorted(set(picked)), np.int64)
    return picked[~np.asarray(unavailable, bool)[picked]]
