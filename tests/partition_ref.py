"""CPU restatement of the CTU partition decision (include/mipgpu.h, mip_partition_device): a
recursive, memoised minimum over split trees, written from the definition -- rectangles and
the split rules, no generated table -- plus an independent legality checker for leaf sets.
Shared by tests/test_partition_cpu.py and tests/test_gpu_partition.py."""
from functools import lru_cache

import numpy as np

from mipgpu import layout

INF = None                     # a region that cannot be tiled
UNAVAILABLE = layout.UNAVAILABLE
MAX_LEAVES = 1024
MAX_BT_DEPTH = 3
LEAF, BT_H, BT_V, TT_H, TT_V, QT = range(6)   # candidate order


@lru_cache(maxsize=None)
def cu_lookup():
    """(x, y, w, h) inside the CTU -> (CU index inside the CTU, shape index)."""
    shape, x, y = layout._ctu_cus()
    return {(int(x[k]), int(y[k]), layout.SHAPES[shape[k]].w, layout.SHAPES[shape[k]].h): (k, int(shape[k]))
            for k in range(layout.CUS_PER_CTU)}


def bt_splits(x, y, w, h):
    """(candidate, children) of the binary / ternary splits a w x h rectangle allows."""
    out = []
    if h >= 8:
        out.append((BT_H, [(x, y, w, h // 2), (x, y + h // 2, w, h // 2)]))
    if w >= 8:
        out.append((BT_V, [(x, y, w // 2, h), (x + w // 2, y, w // 2, h)]))
    if h >= 16:
        out.append((TT_H, [(x, y, w, h // 4), (x, y + h // 4, w, h // 2), (x, y + 3 * h // 4, w, h // 4)]))
    if w >= 16:
        out.append((TT_V, [(x, y, w // 4, h), (x + w // 4, y, w // 2, h), (x + 3 * w // 4, y, w // 4, h)]))
    return out


def quad_children(x, y, s):
    return [(x + i * s // 2, y + j * s // 2, s // 2, s // 2) for j in (0, 1) for i in (0, 1)]


def enumerate_states():
    """Every state the rules reach in one CTU: the set of quad-tree nodes (x, y, side) and the set of
    binary/ternary states (x, y, w, h, depth) (nodes of side <= 32 are the depth-0 ones)."""
    quads, states = set(), set()

    def bt(r, d):
        if r + (d,) in states:
            return
        states.add(r + (d,))
        if d < MAX_BT_DEPTH:
            for _, ch in bt_splits(*r):
                for c in ch:
                    bt(c, d + 1)

    def quad(x, y, s):
        quads.add((x, y, s))
        if s <= 32:
            bt((x, y, s, s), 0)
        if s >= 16:
            for c in quad_children(x, y, s):
                quad(c[0], c[1], c[2])

    quad(0, 0, 128)
    return quads, states


def partition_ctu(cost, penalty, width, height, cx, cy):
    """Minimum-cost partition of the CTU at (cx, cy): cost = the CTU's 5380 best costs, penalty[47].
    Returns (total or None, sorted list of leaf CU indices inside the CTU)."""
    cus = cu_lookup()
    memo = {}

    def leaf_cost(r):
        x, y, w, h = r
        if r not in cus or cx + x + w > width or cy + y + h > height:
            return INF
        k, s = cus[r]
        return INF if cost[k] == UNAVAILABLE else int(cost[k]) + int(penalty[s])

    def split_cost(values):
        total = 0
        for v, _ in values:
            if v is INF:
                return INF
            total += v
        return total

    def best(r, d, node):
        """(cost, leaves) of region r: node = quad-tree node (d == 0 then), else BT state at depth d."""
        key = (r, d, node)
        if key in memo:
            return memo[key]
        x, y, w, h = r
        if cx + x >= width or cy + y >= height:
            res = (0, ())
        else:
            cands = []
            if not (node and w == 128):
                cands.append((leaf_cost(r), (cus[r][0],) if r in cus else ()))
            if w <= 32 and d < MAX_BT_DEPTH:
                for _, ch in bt_splits(*r):
                    parts = [best(c, d + 1, False) for c in ch]
                    cands.append((split_cost(parts), sum((p[1] for p in parts), ())))
            if node and w >= 16:
                parts = [best(c, 0, True) for c in quad_children(x, y, w)]
                cands.append((split_cost(parts), sum((p[1] for p in parts), ())))
            res = (INF, ())
            for c, leaves in cands:      # candidate order; strictly cheaper replaces
                if c is not INF and (res[0] is INF or c < res[0]):
                    res = (c, leaves)
        memo[key] = res
        return res

    total, leaves = best((0, 0, 128, 128), 0, True)
    return total, sorted(leaves)


def as_penalty(penalty):
    if penalty is None:
        return np.zeros(layout.NUM_SHAPES, np.int64)
    p = np.asarray(penalty, np.int64)
    return np.full(layout.NUM_SHAPES, int(p), np.int64) if p.ndim == 0 else p


def partition_frames(best_cost, width, height, penalty=None, best_mode=None):
    """All four outputs of mip_partition_device for best_cost [F, nCTUs*5380] as numpy arrays:
    dict(leaf uint8 [F, nCTUs*5380], ctu_cost, ctu_leaves int32 [F, nCTUs], and -- with best_mode --
    items, a mipgpu.PRED_ITEM array [F, nCTUs, 1024])."""
    import mipgpu
    bc = np.asarray(best_cost).reshape(-1, layout.num_ctus(width, height), layout.CUS_PER_CTU)
    nf, nctus, _ = bc.shape
    cols, _ = layout.ctu_grid(width, height)
    pen = as_penalty(penalty)
    _, lx, ly = layout._ctu_cus()
    leaf = np.zeros((nf, nctus, layout.CUS_PER_CTU), np.uint8)
    ctu_cost = np.zeros((nf, nctus), np.int32)
    ctu_leaves = np.zeros((nf, nctus), np.int32)
    items = None
    if best_mode is not None:
        bm = np.asarray(best_mode).reshape(bc.shape)
        items = np.zeros((nf, nctus, MAX_LEAVES), mipgpu.PRED_ITEM)
        items["frame"] = items["cu"] = items["mode"] = -1
    for f in range(nf):
        for c in range(nctus):
            cx, cy = 128 * (c % cols), 128 * (c // cols)
            total, leaves = partition_ctu(bc[f, c], pen, width, height, cx, cy)
            if total is INF:
                ctu_cost[f, c] = UNAVAILABLE
                continue
            ctu_cost[f, c] = total
            ctu_leaves[f, c] = len(leaves)
            leaf[f, c, leaves] = 1
            if items is not None:
                it = items[f, c, :len(leaves)]
                k = np.asarray(leaves, np.int64)
                it["frame"], it["cu"], it["mode"], it["pitch"] = f, c * layout.CUS_PER_CTU + k, bm[f, c, k], width
                it["offset"] = f * width * height + (cy + ly[k].astype(np.int64)) * width + cx + lx[k]
    out = dict(leaf=leaf.reshape(nf, -1), ctu_cost=ctu_cost, ctu_leaves=ctu_leaves)
    if items is not None:
        out["items"] = items
    return out


def is_legal_partition(leaf_cus, width, height, cx, cy):
    """Independent check of a leaf set (CU indices inside the CTU at (cx, cy)): the leaves are
    CUs wholly inside the frame, pairwise disjoint, cover the in-frame part of the CTU, and SOME
    split tree under the rules has exactly them as leaves."""
    shape, lx, ly = layout._ctu_cus()
    rects = set()
    covered = np.zeros((128, 128), np.int32)
    for k in leaf_cus:
        s = layout.SHAPES[shape[k]]
        x, y = int(lx[k]), int(ly[k])
        if cx + x + s.w > width or cy + y + s.h > height:
            return False
        covered[y:y + s.h, x:x + s.w] += 1
        rects.add((x, y, s.w, s.h))
    inside = np.zeros((128, 128), np.int32)
    inside[:max(0, min(128, height - cy)), :max(0, min(128, width - cx))] = 1
    if len(rects) != len(list(leaf_cus)) or not np.array_equal(covered, inside):
        return False

    @lru_cache(maxsize=None)
    def tiles(r, d, node):
        x, y, w, h = r
        if cx + x >= width or cy + y >= height:
            return True                      # (coverage above: no leaf reaches in here)
        if r in rects:
            return not (node and w == 128) and (w <= 32 or node)
        if w <= 32 and d < MAX_BT_DEPTH and any(all(tiles(c, d + 1, False) for c in ch) for _, ch in bt_splits(*r)):
            return True
        return bool(node and w >= 16 and all(tiles(c, 0, True) for c in quad_children(x, y, w)))

    return tiles((0, 0, 128, 128), 0, True)
