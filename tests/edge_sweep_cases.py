"""Inputs and references of the residue sweep through the intra, angular, refined angular, merge,
partition, predict and candidate kernels (tests/test_gpu_edge_sweep.py,
tests/test_gpu_angular_sweep.py, tests/test_gpu_refine_sweep.py) -- a helper, not a test.  The
sizes are tests/size_sweep.py's; every reference is one of the independent restatements
(tests/intra_ref.py, tests/angular_ref.py, tests/angular_refine_ref.py, tests/candidates_ref.py,
tests/partition_ref.py, tests/predict_ref.py, the C oracle), computed once (lru_cache) and shared;
callers do not modify the arrays."""
from functools import lru_cache

import numpy as np

import angular_ref as A
import angular_refine_ref as RR
import candidates_ref as K
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


def angular_sweep_case(w, h, kind="noise", filt=None, modes=SWEEP_MODES):
    """(frame [H, W], references, availability set, dict of the tables of tests/angular_ref.py
    [nCTUs*5380, 65] plus 'ang_mode' / 'ang_cost' [nCTUs*5380]) of intra_case's frame for the mode
    list `modes` (a tuple; None: all 65): the frame, the oracle's filter and the set are
    intra_case's own, computed once for all sweeps (one cache entry however the arguments are
    spelled)."""
    return _angular_sweep_case(w, h, kind, filt, None if modes is None else tuple(modes))


@lru_cache(maxsize=None)
def _angular_sweep_case(w, h, kind, filt, modes):
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


# ---------------------------------------------------------------- the refined angular kernel's sweep
# (list, seeds) of sweep size i is REFINE_ROTATION[i % 7].  The list of one mode has
# nmodes == nseeds (the launcher's limit case) and a coarse round that is half empty; with (2, 66)
# every candidate is 3 or 65.  tests/test_gpu_refine_sweep.py holds the rotation to what it reaches.
REFINE_ROTATION = ((SWEEP_MODES, 1), (RR.EVEN_MODES, 2), (RR.ODD_MODES, 3), ((34,), 1), (RR.SPARSE_MODES, 3), ((2, 66), 2),
                   (RR.EVEN_MODES, 1))
# On a noise frame with original references every boundary of the CUs at (0, 0) is the 512
# substitute and all modes tie: the seeds are 17, 19, 49, the candidates 16, 18, 20, 48, 50 -- both
# PDPC modes as per-lane candidates on substituted lines -- and mode 16 wins with 9 modes tried.
PDPC_TIE_CONFIG = ((17, 19, 49, 51), 3)
PDPC_TIE_SIZES = ((148, 148), (20, 20), (124, 4))
OTHER_CONFIG = (RR.EVEN_MODES, 2)                              # of the six filters at OTHER_SIZE
# the candidate chain: Planar / DC and the refined angular stage, as tests/test_gpu_candidates.py
CAND_K, CAND_ANGULAR, CAND_INTRA_BIAS, CAND_ANGULAR_BIAS = 3, (RR.EVEN_MODES, 2), (3, 5), 9
# the host calls' cut case (tests/test_gpu_angular_sweep.py's): 200 one-CTU frames of period 3
CUT_SIZE, CUT_FRAMES, CUT_PERIOD = (60, 52), 200, 3
TABLE_BYTES = 256 << 20                                        # kAngularTableBytes of csrc/host_policy.h


def refine_config(size):
    """(list, seeds) of a sweep size, by its index in tests/size_sweep.py; OTHER_CONFIG at OTHER_SIZE."""
    return OTHER_CONFIG if size == OTHER_SIZE else REFINE_ROTATION[S.ALL_SIZES.index(size) % len(REFINE_ROTATION)]


@lru_cache(maxsize=None)
def refine_sweep_case(w, h, kind, filt, modes, seeds):
    """(frame, references, availability set, tests/angular_refine_ref.py's refine) of
    angular_sweep_case(w, h, kind, filt, None)'s 65-mode tables for the list `modes` (a tuple) and
    `seeds`."""
    frame, refs, un, tabs = angular_sweep_case(w, h, kind, filt, None)
    out = RR.refine({k: tabs[k] for k in TABLES}, modes, seeds)
    _freeze(*out.values())
    return frame, refs, un, out


def candidate_wins(r):
    """bool per CU of a refine result: the ang pair's mode is one of the CU's candidates."""
    slot = np.clip(r["ang_mode"].astype(int) - A.MODE_BASE - A.FIRST, 0, A.MODES - 1)
    return (r["tried"] > 0) & np.take_along_axis(r["cand"], slot[..., None], axis=-1)[..., 0]


REFINE_CONDITIONS = ("pdpc_first_column", "pdpc_first_row", "wins_wrapped", "wins_first_column", "wins_first_row", "big_full", "big_fewer",
                     "big_mixed_sizes", "end_candidates")


def refine_conditions(w, h, modes, seeds, r, un):
    """What the refined sweep is about, counted for one size from the restatement `r` alone: dict
    of REFINE_CONDITIONS -> CUs (big_mixed_sizes: 1 if the launch holds an available and an
    unavailable 64x64 CU)."""
    x, y, bw, bh = geometry(w, h)
    ok, cand = ~un, r["cand"]
    pdpc = ok & (cand[:, 18 - A.FIRST] | cand[:, 50 - A.FIRST])
    wins = candidate_wins(r)
    big = (bw == 64) & (bh == 64)
    n = cand.sum(axis=-1)
    full = 2 * min(seeds, len(modes))
    return {"pdpc_first_column": int((pdpc & (x == 0) & (y > 0)).sum()), "pdpc_first_row": int((pdpc & (y == 0) & (x > 0)).sum()),
            "wins_wrapped": int((wins & wrapped(w, h)).sum()), "wins_first_column": int((wins & (x == 0)).sum()),
            "wins_first_row": int((wins & (y == 0)).sum()), "big_full": int((big & ok & (n == full)).sum()),
            "big_fewer": int((big & ok & (n < full)).sum()), "big_mixed_sizes": int((big & ok).any() and (big & un).any()),
            "end_candidates": int((ok & (cand[:, 0] | cand[:, A.MODES - 1])).sum())}


def table_cut_chunk(bytes_per_frame):
    """Frames per chunk of a host call whose device tables take bytes_per_frame (stage_chunk_frames
    of csrc/host_policy.h for max_batch >= the call's frames)."""
    return TABLE_BYTES // bytes_per_frame


def refine_cut_bytes():
    return layout.num_ctus(*CUT_SIZE) * layout.CUS_PER_CTU * A.MODES * 4     # the cost table; `tried` does not count


def candidates_cut_bytes(k):
    """Per frame of mip_candidates_frames with Planar / DC and angular on a best_k 1 engine: the
    MIP cost table (none for k = 1: the search's own decisions), the Planar / DC table, the angular one."""
    nct = layout.num_ctus(*CUT_SIZE)
    ncu = nct * layout.CUS_PER_CTU
    return (nct * layout.COSTS_PER_CTU * 4 if k > 1 else 0) + ncu * 2 * 4 + ncu * A.MODES * 4


@lru_cache(maxsize=None)
def cut_case():
    """(base frames [3, H, W], availability set, per base frame the refined result (even list, two
    seeds), per base frame the candidate lists (modes, costs) of CAND_K) of the cut case."""
    w, h = CUT_SIZE
    un = mipgpu.unavailable_cus(w, h)
    base = np.stack([S.content("noise", w, h, salt) for salt in range(CUT_PERIOD)])
    nct = layout.num_ctus(w, h)
    fine, lists = [], []
    for f in base:
        r = RR.refine(A.tables(f, f, un), *CAND_ANGULAR)
        mip = layout.topk_modes(O.search(f), nct, CAND_K)
        lists.append(K.candidates(CAND_K, mip[0], mip[1], I.tables(f, f, un)["cost"], CAND_INTRA_BIAS, r["cost"], CAND_ANGULAR_BIAS))
        fine.append(r)
        _freeze(*r.values(), *lists[-1])
    _freeze(base, un)
    return base, un, fine, lists


@lru_cache(maxsize=None)
def candidates_case(w, h, filt=None):
    """(frame, availability set, modes uint8 / costs int32 [nCTUs*5380, CAND_K], the three input
    tables) of the `edges` frame of a size: tests/candidates_ref.py over the C oracle's search as
    lists of CAND_K (layout.topk_modes; with a filter the engine's UNAVAILABLE entries filled in),
    tests/intra_ref.py's table and the refined angular table (CAND_ANGULAR), all on the oracle's
    filter `filt` of the frame with that filter's availability set."""
    frame, _, un, intra = intra_case(w, h, "edges", filt)
    fine = refine_sweep_case(w, h, "edges", filt, *CAND_ANGULAR)[3]
    mip_mode, mip_cost = layout.topk_modes(O.engine_search(frame, filt), layout.num_ctus(w, h), CAND_K)
    modes, costs = K.candidates(CAND_K, mip_mode, mip_cost, intra["cost"], CAND_INTRA_BIAS, fine["cost"], CAND_ANGULAR_BIAS)
    _freeze(modes, costs, mip_mode, mip_cost)
    return frame, un, modes, costs, {"mip_mode": mip_mode, "mip_cost": mip_cost, "intra_cost": intra["cost"], "ang_cost": fine["cost"]}


def family_of(modes):
    """0 MIP, 1 Planar / DC, 2 angular, -1 none, per mode code."""
    modes = np.asarray(modes)
    return np.where(modes < 32, 0, np.where(modes == 0xFF, -1, np.where(modes >= 0xF0, 1, 2)))
