"""Numpy restatement of the coarse-to-fine angular search (mip_angular_refine_device) -- test
helper, not a test.  Written from the contract text in include/mipgpu.h alone, and pure table
work: it takes the 65-mode tables of tests/angular_ref.tables (every mode of every CU) and forms,
per CU, the seeds (the first min(seeds, len(list)) entries of the list sorted by (cost, mode)),
the candidates (their +-1 neighbours inside 2..66 that the list does not hold, as a set), the
evaluated set, the tables masked to it, the ang pair over it and `tried`.  The merge is
angular_ref.merge on that pair.

tests/test_angular_refine_cpu.py pins it by hand-checkable cases; the C++ host walk and the GPU
kernel are compared against it bit for bit.
"""
from __future__ import annotations

import numpy as np

import angular_ref as A

UN = A.UNAVAILABLE
MAX_SEEDS = 3
EVEN_MODES = tuple(range(2, 67, 2))
ODD_MODES = tuple(range(3, 66, 2))
EDGE_MODES = (2, 34, 66)
# both ends of the range, two pairs of modes two apart (a shared neighbour), two adjacent modes (a
# neighbour that is listed), both pure modes
SPARSE_MODES = (2, 10, 12, 18, 19, 33, 35, 50, 58, 66)
TABLES = ("cost", "sad", "satd")


def listed_mask(modes):
    listed = np.zeros(A.MODES, bool)
    listed[np.array(A._modes(modes)) - A.FIRST] = True
    return listed


def seeds_of(cost, modes, seeds):
    """Seed modes int [..., min(seeds, len(modes))] of 65-mode cost tables [..., 65]: the list sorted
    by (cost, mode), its first entries.  (Rows of unavailable CUs are returned too; callers mask.)"""
    modes = np.array(A._modes(modes))
    assert 1 <= seeds <= MAX_SEEDS
    sub = np.asarray(cost, np.int64)[..., modes - A.FIRST]
    order = np.argsort(sub, axis=-1, kind="stable")           # equal costs keep list order: the lower mode first
    return modes[order[..., :min(seeds, modes.size)]]


def candidates(seed_modes, modes):
    """bool [..., 65] by slot: s - 1 and s + 1 of every seed, inside 2..66, not in the list."""
    out = np.zeros(seed_modes.shape[:-1] + (A.MODES,), bool)
    rows = np.indices(seed_modes.shape[:-1])
    for q in range(seed_modes.shape[-1]):
        for step in (-1, 1):
            n = seed_modes[..., q] + step
            ok = (n >= A.FIRST) & (n <= A.LAST)               # no wrap between 2 and 66
            idx = tuple(r[ok] for r in rows) + (n[ok] - A.FIRST,)
            out[idx] = True                                    # (a set: twice is once)
    return out & ~listed_mask(modes)


def refine(tabs, modes, seeds):
    """dict of everything the entry point gives for 65-mode tables `tabs` ('cost', 'sad', 'satd'
    [..., 65], UNAVAILABLE in every slot of an unavailable CU): 'seeds' [..., S], 'cand' and
    'evaluated' bool [..., 65], the masked 'cost' / 'sad' / 'satd', 'ang_mode' / 'ang_cost' and
    'tried' uint8 [...]."""
    cost = np.asarray(tabs["cost"])
    on = cost[..., 0] != UN
    assert np.array_equal(on, (cost != UN).all(axis=-1)) and np.array_equal(~on, (cost == UN).all(axis=-1))
    s = seeds_of(cost, modes, seeds)
    cand = candidates(s, modes) & on[..., None]
    evaluated = (listed_mask(modes) | cand) & on[..., None]
    out = {"seeds": s, "cand": cand, "evaluated": evaluated}
    for k in TABLES:
        out[k] = np.where(evaluated, tabs[k], UN).astype(np.int32)
    out["ang_mode"], out["ang_cost"] = A.best(out["cost"])     # (cost, mode) minimum: the first of equal minima
    out["tried"] = evaluated.sum(axis=-1).astype(np.uint8)
    return out
