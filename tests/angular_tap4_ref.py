"""Numpy restatement of the angular family with VVC's 4-tap luma interpolation (mip_angular_interp,
MIP_ANG_INTERP_4TAP) -- test helper, not a test.  Written from the contract text in
include/mipgpu.h alone: the threshold table T and the choice G, the Gaussian rule fG, the cubic
table fC for f = 0..16 with its reversal, and P = (sum of c[t] * ref[k-1+t] + 32) >> 6 for every f.
Layered on tests/angular_ext_ref.py: its boundaries() give each class's main line with its
extension and, past M', the last sample again -- which is what ref[k] = main[min(k, M') - 1] reads
for every tap -- and lengths 0 / 0 give the substituted lines.  ref[0] is the corner for every
angle; ref[-k] is the side projection with its cap S.

tests/test_angular_tap4_cpu.py pins it by hand-checkable cases; the C++ host walks and the GPU
kernels are compared against it bit for bit.
"""
from __future__ import annotations

import numpy as np

import angular_ext_ref as X
import angular_ref as A
import predict_ref as P
from mipgpu import layout

UNAVAILABLE = A.UNAVAILABLE
INTERP_2TAP, INTERP_4TAP = 0, 1
THRESHOLD = (24, 24, 24, 14, 2, 0, 0)                          # T[(lw + lh) >> 1]
_FC = ((0, 64, 0, 0), (-1, 63, 2, 0), (-2, 62, 4, 0), (-2, 60, 7, -1), (-2, 58, 10, -2), (-3, 57, 12, -2),
       (-4, 56, 14, -2), (-4, 55, 15, -2), (-4, 54, 16, -2), (-5, 53, 18, -2), (-6, 52, 20, -2), (-6, 49, 24, -3),
       (-6, 46, 28, -4), (-5, 44, 29, -4), (-4, 42, 30, -4), (-4, 39, 33, -4), (-4, 36, 36, -4))
FC = np.array([_FC[f] if f <= 16 else _FC[32 - f][::-1] for f in range(32)], np.int64)          # [32, 4]
FG = np.array([(16 - (f >> 1), 32 - (f >> 1), 16 + (f >> 1), f >> 1) for f in range(32)], np.int64)
FRACTIONAL_MODES = tuple(m for m in A.ALL_MODES if m not in (2, 18, 34, 50, 66))                # the 60 modes with a fractional angle


def filter_gauss(lw, lh, m):
    """G of the contract: True where the CU takes the Gaussian table for mode m."""
    return min(abs(m - 50), abs(m - 18)) > THRESHOLD[(lw + lh) >> 1]


def predict(top, left, corner, w, h, modes=None, pdpc=True, clip=True, want=None):
    """The predicted blocks, int64 [len(modes), n, h, w], of angular_ext_ref.boundaries() lines
    top [n, w + h], left [n, h + w], corner [n].  pdpc / clip as in angular_ref.predict.  want: an
    optional dict that receives, per mode, 'k' and 'pos' -- the four taps' reference indexes k-1 .. k+2
    and their positions in base[] (below), int64 [4, h, w] (the same for every CU) --, 'f' [h, w] and
    'S', 'M', 'inv'; for the coverage tests."""
    modes = A._modes(modes)
    top, left, corner = np.asarray(top, np.int64), np.asarray(left, np.int64), np.asarray(corner, np.int64)
    assert top.shape[1] == w + h and left.shape[1] == h + w
    lw, lh = A._log2(w), A._log2(h)
    i, j = np.broadcast_to(np.arange(w)[None, :], (h, w)), np.broadcast_to(np.arange(h)[:, None], (h, w))
    out = np.empty((len(modes), top.shape[0], h, w), np.int64)
    for q, m in enumerate(modes):
        ang = A.ANGLE[m]
        if m >= 34:
            main, side, a, b = top, left[:, :h], i, j
        else:
            main, side, a, b = left, top[:, :w], j, i
        M, S = main.shape[1], side.shape[1]                   # (M = M + S here: past M' the line repeats its last sample)
        # base[S - t] = side'[t] (t = 0..S, side'[0] = corner), base[S + u] = main[u - 1] (u = 1..M)
        base = np.concatenate([side[:, ::-1], corner[:, None], main], axis=1)
        inv = A.INVERSE[abs(ang)] if ang else 0

        def position(k):
            t = np.minimum((-k * inv + 256) >> 9, S)          # (used for k < 0, reached only with A < 0)
            assert ang < 0 or np.all(k >= 0)
            return np.where(k >= 1, S + np.minimum(k, M), np.where(k == 0, S, S - t))

        d = (b + 1) * ang
        idx, f = d >> 5, d & 31
        k = a + idx + 1
        c = (FG if filter_gauss(lw, lh, m) else FC)[f]        # [h, w, 4]
        pos = np.stack([position(k - 1 + t) for t in range(4)])
        p = (sum(c[:, :, t] * base[:, pos[t]] for t in range(4)) + 32) >> 6
        if want is not None:
            want[m] = {"pos": pos, "k": np.stack([k - 1 + t for t in range(4)]), "S": S, "M": M, "inv": inv, "f": f}
        if pdpc and m in (18, 50):
            scale = (lw + lh - 2) >> 2
            cc = corner[:, None, None]
            if m == 50:
                wl, wt = A.weight(i, scale), 0
                ref_l, ref_t = left[:, :h, None] - cc + p, 0
            else:
                wl, wt = 0, A.weight(j, scale)
                ref_l, ref_t = 0, top[:, None, :w] - cc + p
            p = (ref_l * wl + ref_t * wt + (64 - wl - wt) * p + 32) >> 6
        out[q] = np.clip(p, 0, 1023) if pdpc and clip else p
    return out


def tables(frame, refs, unavailable, e_top=None, e_left=None, modes=None):
    """angular_ext_ref.tables with the 4-tap predictor; e_top / e_left None: the substituted lines."""
    modes = A._modes(modes)
    height, width = frame.shape
    ncu = layout.num_ctus(width, height) * layout.CUS_PER_CTU
    unavailable = np.asarray(unavailable, bool)
    assert unavailable.shape == (ncu,)
    e_top = np.zeros(ncu, np.int64) if e_top is None else np.asarray(e_top, np.int64)
    e_left = np.zeros(ncu, np.int64) if e_left is None else np.asarray(e_left, np.int64)
    shape, x, y, _, _ = layout.cu_geometry(width, height, np.arange(ncu))
    sad = np.full((ncu, A.MODES), UNAVAILABLE, np.int64)
    satd = sad.copy()
    flat = np.asarray(frame).reshape(-1).astype(np.int64)
    slots = np.array(modes) - A.FIRST
    for s in layout.SHAPES:
        k = np.nonzero((shape == s.index) & ~unavailable)[0]
        if not k.size:
            continue
        top, left, corner = X.boundaries(refs, x[k], y[k], s.w, s.h, e_top[k], e_left[k])
        idx = (y[k, None, None] + np.arange(s.h)[None, :, None]).astype(np.int64) * width + x[k, None, None] + np.arange(s.w)[None, None, :]
        orig = flat[idx]
        blocks = predict(top, left, corner, s.w, s.h, modes)
        sad[k[:, None], slots[None, :]] = P.sad_blocks(orig[None], blocks).T
        satd[k[:, None], slots[None, :]] = P.satd_blocks(orig[None], blocks).T
    cost = np.where(sad == UNAVAILABLE, UNAVAILABLE, np.minimum(2 * sad, satd))
    return {"cost": cost.astype(np.int32), "sad": sad.astype(np.int32), "satd": satd.astype(np.int32)}


def predict_cu(refs, x, y, w, h, e_top, e_left, mode):
    """The block [h, w] uint16 of ONE CU and one mode number."""
    top, left, corner = X.boundaries(refs, [x], [y], w, h, [e_top], [e_left])
    return predict(top, left, corner, w, h, (mode,))[0, 0].astype(np.uint16)
