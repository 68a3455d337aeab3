"""Inputs and references of the residue sweep through the intra, angular, merge, partition and
predict kernels (tests/test_gpu_edge_sweep.py, tests/test_gpu_angular_sweep.py) -- a helper, not a
test.  The sizes are tests/size_sweep.py's; every reference is one of the independent restatements
(tests/intra_ref.py, tests/angular_ref.py, tests/partition_ref.py, tests/predict_ref.py, the C
oracle), computed once (lru_cache) and shared; callers do not modify the arrays."""
from functools import lru_cache

import numpy as np

import angular_ref as A
import intra_ref as I
import mipgpu
import oracle_lib as O
import partition_ref as R
import predict_ref as P
import size_sweep as S
from mipgpu import layout

UN = layout.UNAVAILABLE
TABLES = ("cost", "sad", "satd")
FILTER_SEP = "filterFrame_1d_int"
FILTER_2D = "filterFrame_2d_float_5x5_quarterCtu"
FIFTH = S.ALL_SIZES[::5]                                      # 14 sizes: 7 of family A, 6 of B, 1 of C
OTHER_FILTERS = [f for f in mipgpu.FILTERS if f not in (FILTER_SEP, FILTER_2D)]
OTHER_SIZE = (136, 72)                                        # where the six other filters run once each
# per-shape penalty of the partition sweep: all of 0 .. 1<<20, no two shapes alike
VECTOR_PENALTY = tuple(int(v) for v in (np.arange(layout.NUM_SHAPES) * 21845) % ((1 << 20) + 1))
CHAIN_BIAS = (30, 30)
CHAIN_PENALTY = 600
FILL = 0xFFFF                                                 # canvas samples nothing wrote


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def geometry(w, h):
    """x, y, w, h of every CU of a frame."""
    _, x, y, bw, bh = layout.cu_geometry(w, h, np.arange(layout.num_ctus(w, h) * layout.CUS_PER_CTU))
    return x, y, bw, bh


def wrapped(w, h):
    """CUs that reach past the frame's right edge: their samples wrap into the next rows."""
    x, _, bw, _ = geometry(w, h)
    return x + bw > w


@lru_cache(maxsize=None)
def intra_case(w, h, kind="noise", filt=None):
    """(frame [H, W], references, availability set, tables of tests/intra_ref.py) of one sweep
    frame: the references are the originals or the oracle's filter `filt` of them (kernel index 0),
    the set is mip_unavailable_cus of that source -- the CUs that read a sample the reference's
    filter takes from past the frame's end are unavailable, racing stores get the owning tile's
    value in the oracle as in the engine, as in
    tests/test_gpu_size_sweep.py."""
    frame = S.content(kind, w, h)
    refs = frame if filt is None else O.filter_frame(frame, filt, 0)
    un = mipgpu.unavailable_cus(w, h, filt)
    tabs = I.tables(frame, refs, un)
    _freeze(frame, refs, un, *tabs.values())
    return frame, refs, un, tabs


def max_boundary(refs, un, w, h):
    """Largest boundary sample over the available CUs of refs [H, W]: above 1023 means the PDPC
    clip has something to do."""
    flat = refs.reshape(-1).astype(np.int64)
    x, y, bw, bh = geometry(w, h)
    best = 0
    for k in np.nonzero(~un)[0]:
        if y[k] > 0:
            best = max(best, flat[(y[k] - 1) * w + x[k]:(y[k] - 1) * w + x[k] + bw[k]].max(initial=0))
        if x[k] > 0:
            best = max(best, flat[y[k] * w + x[k] - 1:(y[k] + bh[k]) * w + x[k] - 1:w].max(initial=0))
    return int(best)


@lru_cache(maxsize=None)
def partition_case(w, h):
    """(best_cost int32 [1, ncu], best_mode uint8 [1, ncu], partition_ref's outputs): per CU the
    cheaper of the Planar and the DC cost of intra_case(w, h), unavailable CUs kept, under
    VECTOR_PENALTY."""
    _, _, un, tabs = intra_case(w, h)
    cost = tabs["cost"].min(axis=1)
    mode = np.where(un, 0xFF, np.where(tabs["cost"][:, 1] < tabs["cost"][:, 0], I.MODE_DC, I.MODE_PLANAR)).astype(np.uint8)
    assert np.array_equal(cost == UN, un)
    cost, mode = cost[None].astype(np.int32), mode[None]
    ref = R.partition_frames(cost, w, h, VECTOR_PENALTY, best_mode=mode)
    _freeze(cost, mode, *ref.values())
    return cost, mode, ref


@lru_cache(maxsize=None)
def chain_case(w, h):
    """Everything the device chain search -> merge -> partition -> predict must give for the
    `edges` frame of a size, original references: dict of the frame, the oracle's argmin
    (mip_mode, mip_cost), the merged decisions (best_mode, best_cost), partition_ref's outputs and
    the expected canvas (MIP leaves predicted by tests/predict_ref.py, everything else FILL)."""
    frame, _, un, tabs = intra_case(w, h, "edges")
    nct = layout.num_ctus(w, h)
    mip_mode, mip_cost = layout.best_modes(O.search(frame), nct)
    assert np.array_equal(mip_cost == UN, un)
    mode, cost = I.merge(mip_mode[None], mip_cost[None], tabs["cost"][None], CHAIN_BIAS)
    ref = R.partition_frames(cost, w, h, CHAIN_PENALTY, best_mode=mode)
    leaf = ref["leaf"][0].astype(bool)
    regular = leaf & ((mode[0] == I.MODE_PLANAR) | (mode[0] == I.MODE_DC))
    canvas = np.full((h, w), FILL, np.uint16)
    ks = np.nonzero(leaf & ~regular)[0]
    shape, x, y, bw, bh = layout.cu_geometry(w, h, ks)
    for i, k in enumerate(ks):
        canvas[y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] = P.CuPredictor(frame, x[i], y[i], shape[i]).predict(mode[0, k])
    out = dict(frame=frame, mip_mode=mip_mode[None], mip_cost=mip_cost[None], best_mode=mode, best_cost=cost, leaf=leaf,
               regular=regular, canvas=canvas, **{k: ref[k] for k in ("ctu_cost", "ctu_leaves", "items")})
    _freeze(*out.values())
    return out


# ---------------------------------------------------------------- the angular kernel's sweep
# Both classes, both pure modes (PDPC), both +32 ends, the -32 diagonal, angle -1 and +1 (the
# largest inverse angle), -29 in both classes; an odd count, so the kernel's last round of two
# modes is half empty.  tests/test_gpu_angular_sweep.py asserts these properties from A.ANGLE.
SWEEP_MODES = (2, 10, 18, 19, 26, 33, 34, 35, 42, 50, 51, 58, 66)
# Bias of the angular merge in the chain, after CHAIN_BIAS: over the 14 chain sizes together MIP,
# Planar / DC and angular modes all win CUs and all are leaves (found on the CPU;
# test_angular_chain_inputs_mix_all_three_kinds holds it to that).
ANGULAR_CHAIN_BIAS = 60


@lru_cache(maxsize=None)
def angular_sweep_case(w, h, kind="noise", filt=None, modes=SWEEP_MODES):
    """(frame [H, W], references, availability set, dict of the tables of tests/angular_ref.py
    [nCTUs*5380, 65] plus 'ang_mode' / 'ang_cost' [nCTUs*5380]) of intra_case's frame for the mode
    list `modes` (a tuple; None: all 65): the frame, the oracle's filter and the set are
    intra_case's own, computed once for both sweeps."""
    frame, refs, un, _ = intra_case(w, h, kind, filt)
    tabs = A.tables(frame, refs, un, modes)
    tabs["ang_mode"], tabs["ang_cost"] = A.best(tabs["cost"])
    _freeze(*tabs.values())
    return frame, refs, un, tabs


def boundary_sets(refs, un, w, h):
    """[(shape, CU indexes, top, left, corner)] of tests/angular_ref.py's boundaries for the
    available CUs of refs [H, W], one entry per shape that has any."""
    shape, x, y, _, _ = layout.cu_geometry(w, h, np.arange(un.size))
    out = []
    for s in layout.SHAPES:
        k = np.nonzero((shape == s.index) & ~un)[0]
        if k.size:
            out.append((s, k) + A.boundaries(refs, x[k], y[k], s.w, s.h))
    return out


def max_boundary_or_corner(refs, un, w, h):
    """Largest boundary or corner sample over the available CUs of refs [H, W]."""
    return max(int(max(top.max(), left.max(), corner.max())) for _, _, top, left, corner in boundary_sets(refs, un, w, h))


def pdpc_range(refs, un, w, h):
    """(lowest, highest) value of modes 18 and 50 before the clip, over the available CUs."""
    lo, hi = 1 << 30, -(1 << 30)
    for s, _, top, left, corner in boundary_sets(refs, un, w, h):
        p = A.predict(top, left, corner, s.w, s.h, (18, 50), clip=False)
        lo, hi = min(lo, int(p.min())), max(hi, int(p.max()))
    return lo, hi


def projection(bw, bh, m):
    """(k, p, S) of a negative-angle mode m on a bw x bh CU: every index k the predictor asks
    ref[] for (a + idx + 1, and a + idx + 2 where the fraction is not 0, as A.predict does), the
    side projection p = (-k * inv + 256) >> 9 of each, and the side's length S."""
    ang = A.ANGLE[m]
    assert ang < 0
    i, j = np.meshgrid(np.arange(bw), np.arange(bh))
    a, b, S = (i, j, bh) if m >= 34 else (j, i, bw)
    d = (b + 1) * ang
    k = np.concatenate([(a + (d >> 5) + 1).reshape(-1), (a + (d >> 5) + 2)[(d & 31) != 0]])
    return k, (-k * A.INVERSE[-ang] + 256) >> 9, S


@lru_cache(maxsize=None)
def angular_chain_case(w, h):
    """chain_case with the angular merge (SWEEP_MODES, ANGULAR_CHAIN_BIAS) between the Planar / DC
    merge and the partition: dict of the frame, the decisions after the search (mip_*), after the
    Planar / DC merge (intra_*) and after the angular one (best_*), partition_ref's outputs, the
    leaves by kind and the expected canvas -- MIP leaves from tests/predict_ref.py, Planar / DC
    leaves from tests/intra_ref.py, angular leaves FILL."""
    from test_gpu_predict_regular import regular_blocks
    c = chain_case(w, h)
    frame, _, un, tabs = angular_sweep_case(w, h, "edges")
    assert np.array_equal(frame, c["frame"])
    mode, cost = A.merge(c["best_mode"], c["best_cost"], tabs["ang_mode"][None], tabs["ang_cost"][None], ANGULAR_CHAIN_BIAS)
    ref = R.partition_frames(cost, w, h, CHAIN_PENALTY, best_mode=mode)
    leaf = ref["leaf"][0].astype(bool)
    angular = leaf & (mode[0] >= A.MODE_BASE + A.FIRST) & (mode[0] <= A.MODE_BASE + A.LAST)
    regular = leaf & ((mode[0] == I.MODE_PLANAR) | (mode[0] == I.MODE_DC))
    mip = leaf & ~angular & ~regular
    assert np.all(mode[0, mip] < 32)
    canvas = np.full((h, w), FILL, np.uint16)
    ks = np.nonzero(mip | regular)[0]
    shape, x, y, bw, bh = layout.cu_geometry(w, h, ks)
    blocks = regular_blocks(frame, w, h, np.nonzero(regular)[0])
    for i, k in enumerate(ks):
        if regular[k]:
            blk = blocks[int(k)][0 if mode[0, k] == I.MODE_PLANAR else 1]
        else:
            blk = P.CuPredictor(frame, x[i], y[i], shape[i]).predict(mode[0, k])
        canvas[y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] = blk
    out = dict(frame=frame, mip_mode=c["mip_mode"], mip_cost=c["mip_cost"], intra_mode=c["best_mode"], intra_cost=c["best_cost"],
               best_mode=mode, best_cost=cost, leaf=leaf, mip=mip, regular=regular, angular=angular, canvas=canvas,
               **{k: ref[k] for k in ("ctu_cost", "ctu_leaves", "items")})
    _freeze(*out.values())
    return out
