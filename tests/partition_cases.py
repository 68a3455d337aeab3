"""Inputs of the partition tests (tests/test_partition_cpu.py, tests/test_gpu_partition.py):
synthetic per-CU cost arrays and the real-cost chain oracle -> best modes -> partition_ref.
Every reference is computed once (lru_cache) and shared; callers do not modify the arrays."""
from functools import lru_cache

import numpy as np

import partition_ref as R
from mipgpu import layout

SIZES = ((132, 132), (140, 76), (264, 136), (128, 128))
MAX_PENALTY = 1 << 20
# A rate term of the size of the costs themselves: a 4x4 costs up to 2*16*1023 = 32736, so 12000
# per leaf moves the optimum away from the all-4x4 tiling without reaching the all-64x64 one.
MID_PENALTY = 12000
PENALTIES = (0, MID_PENALTY, MAX_PENALTY)


@lru_cache(maxsize=None)
def geometry(width, height):
    """Per CU of a frame: shape, x, y, w, h (frame coordinates) and the geometric
    unavailability of an engine without a filter (layout.cu_defined)."""
    n = layout.num_ctus(width, height) * layout.CUS_PER_CTU
    shape, x, y, w, h = layout.cu_geometry(width, height, np.arange(n))
    un = ~layout.cu_defined(width, height, x.astype(np.int64), y, w, h)
    return shape, x, y, w, h, un


def bound(width, height):
    """The search's largest cost per CU: 2 * w * h * 1023."""
    _, _, _, w, h, _ = geometry(width, height)
    return 2 * w.astype(np.int64) * h * 1023


@lru_cache(maxsize=None)
def costs(width, height, kind, nframes=1, seed=7):
    """(best_cost int32 [F, nCTUs*5380], best_mode uint8 [F, ...]) of one synthetic kind:
    'random'  uniform in 0 .. the search's bound of the CU's shape;
    'ties'    one of four values (1..4) per 4x4 unit of the CU's area, so that a split often costs
              exactly what the leaf or another split costs and the candidate order decides;
    'area'    w*h times a per-CU factor in 600..1299 (known answers, see the test);
    'holes'   'random' with about 5 % of the CUs unavailable.
    CUs an engine without a filter reports unavailable are MIP_COST_UNAVAILABLE / 0xff in all."""
    rng = np.random.default_rng([seed, width, height, nframes, sorted(("random", "ties", "area", "holes")).index(kind)])
    shape, _, _, w, h, un = geometry(width, height)
    n = un.size
    if kind in ("random", "holes"):
        c = rng.integers(0, np.broadcast_to(bound(width, height) + 1, (nframes, n)))
    elif kind == "ties":
        c = rng.integers(1, 5, (nframes, n)) * (w.astype(np.int64) * h // 16)
    else:
        c = rng.integers(600, 1300, (nframes, n)) * (w.astype(np.int64) * h)
    modes = np.array([s.total_modes for s in layout.SHAPES])[shape]
    m = rng.integers(0, np.broadcast_to(modes, (nframes, n)))
    dead = np.broadcast_to(un, (nframes, n)).copy()
    if kind == "holes":
        dead |= rng.random((nframes, n)) < 0.05
    c = np.where(dead, layout.UNAVAILABLE, c).astype(np.int32)
    m = np.where(dead, 0xFF, m).astype(np.uint8)
    for a in (c, m):
        a.setflags(write=False)
    return c, m


def covering(width, height, ctu, x0, y0):
    """CU indices (frame order) of `ctu`'s CUs that cover the CTU-relative sample (x0, y0)."""
    _, lx, ly = layout._ctu_cus()
    shape = layout._ctu_cus()[0]
    ws = np.array([s.w for s in layout.SHAPES])[shape]
    hs = np.array([s.h for s in layout.SHAPES])[shape]
    k = np.nonzero((lx <= x0) & (x0 < lx + ws) & (ly <= y0) & (y0 < ly + hs))[0]
    return ctu * layout.CUS_PER_CTU + k


@lru_cache(maxsize=None)
def impossible(width, height, ctu, nframes=1):
    """'holes' costs in which, in every frame, the 4x4 at (20, 36) of `ctu` and every CU covering
    it are unavailable: that CTU has no partition."""
    c, m = (a.copy() for a in costs(width, height, "holes", nframes))
    kill = covering(width, height, ctu, 20, 36)
    c[:, kill] = layout.UNAVAILABLE
    m[:, kill] = 0xFF
    for a in (c, m):
        a.setflags(write=False)
    return c, m


@lru_cache(maxsize=None)
def reference(width, height, kind, penalty, nframes=1, ctu=None):
    """partition_ref's outputs for costs(...) (ctu given: impossible(...))."""
    c, m = costs(width, height, kind, nframes) if ctu is None else impossible(width, height, ctu, nframes)
    return R.partition_frames(c, width, height, penalty, best_mode=m)


def check_legal(leaf, ctu_cost, ctu_leaves, width, height):
    """Every partition of a leaf output passes the independent legality checker; CTUs without
    a partition have no leaves."""
    cols, _ = layout.ctu_grid(width, height)
    nct = layout.num_ctus(width, height)
    leaf = np.asarray(leaf).reshape(-1, nct, layout.CUS_PER_CTU)
    for f in range(leaf.shape[0]):
        for c in range(nct):
            ks = np.nonzero(leaf[f, c])[0]
            assert ks.size == ctu_leaves.reshape(-1, nct)[f, c]
            if ctu_cost.reshape(-1, nct)[f, c] == layout.UNAVAILABLE:
                assert ks.size == 0
            else:
                assert R.is_legal_partition(ks.tolist(), width, height, 128 * (c % cols), 128 * (c // cols)), (f, c)


# ---- real costs: the oracle's search of synthetic frames -> best modes -> the reference partition
REAL_W, REAL_H, REAL_FRAMES = 264, 136, 3
# (chosen on the CPU: at 1000 per leaf the reference partition mixes 30-odd shapes, NA ones and
# leaves that only the third binary/ternary level reaches; test_partition_cpu.py asserts it)
REAL_PENALTY = 1000


@lru_cache(maxsize=None)
def real_frames():
    from mipgpu.synth import synth_frames
    f = synth_frames(REAL_W, REAL_H, REAL_FRAMES, 0x9A27, 0)
    f.setflags(write=False)
    return f


@lru_cache(maxsize=None)
def real_decisions(filter_name=None):
    """(best_mode, best_cost) [F, nCTUs*5380] of real_frames() by the C oracle, with the engine's
    unavailable CUs (oracle_lib.engine_search); filter_name "caller": the frames in reverse order
    serve as caller-supplied references."""
    import oracle_lib as O
    nct = layout.num_ctus(REAL_W, REAL_H)
    if filter_name == "caller":
        out = [layout.best_modes(O.search(f, r), nct) for f, r in zip(real_frames(), real_frames()[::-1])]
    else:
        out = [layout.best_modes(O.engine_search(f, filter_name), nct) for f in real_frames()]
    bm, bc = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    for a in (bm, bc):
        a.setflags(write=False)
    return bm, bc


@lru_cache(maxsize=None)
def real_reference(filter_name=None):
    bm, bc = real_decisions(filter_name)
    return R.partition_frames(bc, REAL_W, REAL_H, REAL_PENALTY, best_mode=bm)


@lru_cache(maxsize=None)
def min_bt_depth():
    """CU index inside the CTU -> the smallest binary/ternary depth at which the rules reach its
    rectangle (the four 64x64 CUs: 0)."""
    _, states = R.enumerate_states()
    cus = R.cu_lookup()
    depth = np.zeros(layout.CUS_PER_CTU, np.int32) + 99
    for (x, y, w, h, d) in states:
        k = cus[(x, y, w, h)][0]
        depth[k] = min(depth[k], d)
    depth[:4] = 0
    return depth
