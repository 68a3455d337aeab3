"""Case set of the GPU test of the coarse-to-fine angular search
(tests/test_gpu_angular_refine.py) -- test helper, not a test: sizes, lists and seeds, the
restatement's result per case (cached), and the coverage conditions that keep a pass of the GPU
test from being vacuous.  tests/test_angular_refine_cpu.py asserts the conditions without a GPU."""
from functools import lru_cache

import numpy as np

import angular_cases as AC
import angular_ref as A
import angular_refine_ref as RR
from mipgpu import layout

FILTER = AC.FILTER
# (width, height, engine filter): two CTUs with right and bottom residues, one partial CTU
GEOMETRIES = ((136, 72, None), (60, 36, None), (136, 72, FILTER))
LISTS = {"even": RR.EVEN_MODES, "odd": RR.ODD_MODES, "edge": RR.EDGE_MODES, "all": None}
SEEDS = (1, 2, 3)
STRUCTURED = (("x", 50), ("y", 18), ("x-y", 34))


@lru_cache(maxsize=None)
def refined(w, h, filt, name, seeds):
    """RR.refine of the three frames of angular_cases.case(w, h, filt) for LISTS[name]."""
    full = AC.case(w, h, filt)[3]
    out = RR.refine({k: full[k] for k in AC.TABLES}, LISTS[name], seeds)
    for v in out.values():
        v.setflags(write=False)
    return out


def _distinct_sets_in_a_block(w, h, cand):
    """Most distinct candidate sets among the CUs of one shape inside one 32x32 block, over
    cand [frames, ncu, 65]."""
    ncu = cand.shape[1]
    shape, x, y, bw, bh = layout.cu_geometry(w, h, np.arange(ncu))
    small = (bw <= 32) & (bh <= 32)
    cols = layout.ctu_grid(w, h)[0]
    block = ((y // 128 * cols + x // 128) * 16 + (y % 128) // 32 * 4 + (x % 128) // 32) * layout.NUM_SHAPES + shape
    best = 0
    for f in range(cand.shape[0]):
        keys = np.packbits(cand[f], axis=-1)
        keys = [bytes(k) for k in keys]
        groups = {}
        for k in np.nonzero(small & cand[f].any(axis=-1))[0]:
            groups.setdefault(int(block[k]), set()).add(keys[k])
        best = max([best] + [len(v) for v in groups.values()])
    return best


def coverage():
    """The conditions of the GPU test's case set, from the restatement alone: dict of booleans."""
    angle = np.array([A.ANGLE[m] for m in range(2, 67)])
    vertical = np.arange(2, 67) >= 34
    seen = dict.fromkeys(("neg_h", "neg_v", "pos_h", "pos_v", "single_at_end", "shared", "candidate_wins", "list_wins", "eight_sets"), False)
    for w, h, filt in GEOMETRIES:
        for name in LISTS:
            if name == "all":
                continue
            listed = RR.listed_mask(LISTS[name])
            for seeds in SEEDS:
                r = refined(w, h, filt, name, seeds)
                any_cand = r["cand"].any(axis=(0, 1))
                seen["neg_h"] |= bool((any_cand & (angle < 0) & ~vertical).any())
                seen["neg_v"] |= bool((any_cand & (angle < 0) & vertical).any())
                seen["pos_h"] |= bool((any_cand & (angle > 0) & ~vertical).any())
                seen["pos_v"] |= bool((any_cand & (angle > 0) & vertical).any())
                on = r["tried"] > 0
                n = r["cand"].sum(axis=-1)
                at_end = ((r["seeds"] == 2) | (r["seeds"] == 66)).any(axis=-1)
                seen["single_at_end"] |= bool((on & at_end & (n == 1) & (r["seeds"].shape[-1] == 1)).any())
                # a shared neighbour: fewer candidates than two per seed, with no seed at an end and no neighbour listed
                s = r["seeds"]
                if s.shape[-1] > 1:
                    gap2 = (np.abs(s[..., :, None] - s[..., None, :]) == 2).any(axis=(-1, -2))
                    mid = np.zeros(s.shape[:-1], bool)
                    for i in range(s.shape[-1]):
                        for j in range(s.shape[-1]):
                            m = (s[..., i] + s[..., j]) // 2
                            is_mid = (s[..., j] - s[..., i] == 2) & ~listed[np.clip(m - 2, 0, 64)]
                            mid |= is_mid
                    seen["shared"] |= bool((on & gap2 & mid).any())
                won = r["ang_mode"].astype(int) - A.MODE_BASE - 2
                is_cand = np.take_along_axis(r["cand"], np.clip(won, 0, 64)[..., None], axis=-1)[..., 0]
                seen["candidate_wins"] |= bool((on & is_cand).any())
                seen["list_wins"] |= bool((on & ~is_cand).any())
                if not seen["eight_sets"]:
                    seen["eight_sets"] = _distinct_sets_in_a_block(w, h, r["cand"]) >= 8
    return seen
