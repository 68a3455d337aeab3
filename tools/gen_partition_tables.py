#!/usr/bin/env python3
"""Generate vvc-mip-gpu_amd/csrc/partition_tables.h: the state graph of the CTU partition
search (mip_partition_device, contract in include/mipgpu.h) from the CU-shape lattices of
mipgpu/_tables.py.  Needs nothing but this repository.  The header is committed;
tests/test_partition_cpu.py re-renders it byte for byte and compares the expanded graph with
the recursive enumeration of tests/partition_ref.py.

The graph.  A state is a rectangle plus the number of binary/ternary splits already used below
its quad-tree node (depth 0..3).  Every state rectangle lies inside one 32x32 block of the
CTU, and the sixteen blocks are translates of each other: 640 states per block (21 / 114 /
231 / 274 at depth 0..3; the depth-0 ones are the block's quad-tree nodes of side 32, 16, 8).
So the header holds ONE block -- the states in level order, their children per split -- and,
per CU shape, how a CU index moves with the block: cu = cu0 + bx*dx + dy[by].  dy is a table
because the 8x4 / 4x8 "_1half" shapes end at y = 64, where "_2half" (the next shape index,
`hi` = 1) takes over.  The four 64x64 nodes and the CTU root are not in the table.
"""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "vvc-mip-gpu_amd")
DST = os.path.join(PKG, "csrc", "partition_tables.h")

MAX_DEPTH = 3
NONE = 0xFFFF


def shapes():
    spec = importlib.util.spec_from_file_location("_mip_tables", os.path.join(PKG, "mipgpu", "_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SHAPES


def _axis(base, step, dual, n):
    if dual:
        return [base + (i // 2) * step + (i % 2) * dual for i in range(n)]
    return [base + i * step for i in range(n)]


def cu_map():
    """(x, y, w, h) inside the CTU -> (CU index inside the CTU, shape index)."""
    out, k = {}, 0
    for si, (_, w, h, _, _, ncols, nrows, ncu, xb, xs, xd, yb, ys, yd, _) in enumerate(shapes()):
        xv, yv = _axis(xb, xs, xd, ncols), _axis(yb, ys, yd, nrows)
        for cu in range(ncu):
            key = (xv[cu % ncols], yv[cu // ncols], w, h)
            assert key not in out, key
            out[key] = (k, si)
            k += 1
    assert k == 5380
    return out


def bt_children(x, y, w, h):
    """Children of the four binary/ternary splits (BT-H, BT-V, TT-H, TT-V); None = not allowed."""
    return [
        [(x, y, w, h // 2), (x, y + h // 2, w, h // 2)] if h >= 8 else None,
        [(x, y, w // 2, h), (x + w // 2, y, w // 2, h)] if w >= 8 else None,
        [(x, y, w, h // 4), (x, y + h // 4, w, h // 2), (x, y + 3 * h // 4, w, h // 4)] if h >= 16 else None,
        [(x, y, w // 4, h), (x + w // 4, y, w // 2, h), (x + 3 * w // 4, y, w // 4, h)] if w >= 16 else None,
    ]


def qt_children(x, y, s):
    return [(x + i * s // 2, y + j * s // 2, s // 2, s // 2) for j in (0, 1) for i in (0, 1)]


def block_states():
    """States (x, y, w, h, depth) of the 32x32 block at the origin, level order: the nodes of
    side 32, 16, 8 (raster), then depth 1, 2, 3 (each sorted by y, x, h, w)."""
    nodes = [(0, 0, 32, 32)]
    nodes += [(x, y, 16, 16) for y in range(0, 32, 16) for x in range(0, 32, 16)]
    nodes += [(x, y, 8, 8) for y in range(0, 32, 8) for x in range(0, 32, 8)]
    levels = [[n + (0,) for n in nodes]]
    for d in range(MAX_DEPTH):
        nxt = set()
        for (x, y, w, h, _) in levels[d]:
            for ch in bt_children(x, y, w, h):
                for c in ch or []:
                    nxt.add(c + (d + 1,))
        levels.append(sorted(nxt, key=lambda s: (s[1], s[0], s[3], s[2])))
    return levels


def template():
    """The block template: dict with states [(x, y, w, h, depth, cu0, shape)], level begins,
    child [[10 state indices]], qt [[4]], step {shape: (dx, dy[4], hi)}."""
    cus = cu_map()
    levels = block_states()
    states = [s for lv in levels for s in lv]
    index = {s: i for i, s in enumerate(states)}
    begins = [0, 1, 5, 21]
    for lv in levels[1:]:
        begins.append(begins[-1] + len(lv))
    nsplit = begins[-2]
    child = []
    for (x, y, w, h, d) in states[:nsplit]:
        row = []
        for ch, n in zip(bt_children(x, y, w, h), (2, 2, 3, 3)):
            row += [index[c + (d + 1,)] for c in ch] if ch else [NONE] * n
        child.append(row)
    qt = [[index[c + (0,)] for c in qt_children(x, y, w)] for (x, y, w, h, d) in states[:5]]
    # how the CU index of a state's rectangle moves with the block
    step = {}
    full = []
    for (x, y, w, h, d) in states:
        cu0, sh = cus[(x, y, w, h)]
        at = {(bx, by): cus[(x + 32 * bx, y + 32 * by, w, h)] for by in range(4) for bx in range(4)}
        dx = at[(1, 0)][0] - cu0
        dy = tuple(at[(0, by)][0] - cu0 for by in range(4))
        hi = at[(0, 2)][1] - sh
        assert hi in (0, 1)
        for (bx, by), (cu, s2) in at.items():
            assert cu == cu0 + bx * dx + dy[by] and s2 == sh + (hi if by >= 2 else 0), (x, y, w, h, bx, by)
        assert step.setdefault(sh, (dx, dy, hi)) == (dx, dy, hi)
        full.append((x, y, w, h, d, cu0, sh))
    return dict(states=full, begins=begins, nsplit=nsplit, child=child, qt=qt, step=step)


def expand_ctu(t=None):
    """Every binary/ternary state of a CTU from the template: [(x, y, w, h, depth, cu, shape)],
    index block*640 + local (block = 4*by + bx), and the children as global indices."""
    t = t or template()
    n = len(t["states"])
    out, kids = [], []
    for b in range(16):
        bx, by = b % 4, b // 4
        for i, (x, y, w, h, d, cu0, sh) in enumerate(t["states"]):
            dx, dy, hi = t["step"][sh]
            out.append((x + 32 * bx, y + 32 * by, w, h, d, cu0 + bx * dx + dy[by], sh + (hi if by >= 2 else 0)))
            row = [(-1 if c == NONE else b * n + c) for c in t["child"][i]] if i < t["nsplit"] else [-1] * 10
            row += [b * n + c for c in t["qt"][i]] if i < 5 else [-1] * 4
            kids.append(row)
    return out, kids


def render():
    t = template()
    st, b = t["states"], t["begins"]
    assert len(st) == 640 and b == [0, 1, 5, 21, 135, 366, 640], (len(st), b)
    o = []
    o.append("/* GENERATED by tools/gen_partition_tables.py -- do not edit.\n"
             " * State graph of the CTU partition search (include/mipgpu.h, mip_partition_device) for ONE\n"
             " * 32x32 block of a CTU; the sixteen blocks are translates of each other.  Plain C99.\n"
             " * A state is a CU rectangle plus the binary/ternary depth already used (0..3); states are\n"
             " * listed in level order: the quad-tree nodes of side 32, 16 (4), 8 (16) -- depth 0 -- then\n"
             " * depth 1, 2, 3.  MIP_PART_LEVELS holds the first state of each of these six groups and the\n"
             " * end.  State s of block (bx, by) is CU  cu0 + bx*step.dx + step.dy[by]  of the CTU, of shape\n"
             " * shape + (by >= 2 ? step.hi : 0), step = MIP_PART_STEP_TABLE[shape], at (32*bx + x, 32*by + y).\n"
             " * MIP_PART_CHILD_TABLE[s], s < MIP_PART_SPLIT_STATES (depth < 3): the child states (same block)\n"
             " * of BT-H [0..1], BT-V [2..3], TT-H [4..6], TT-V [7..9]; 0xffff = split not allowed.\n"
             " * MIP_PART_QT_TABLE[s], s < MIP_PART_QT_STATES: the four quad-split children. */")
    o.append("#ifndef MIPGPU_PARTITION_TABLES_H\n#define MIPGPU_PARTITION_TABLES_H\n#include <stdint.h>\n")
    o.append("#define MIP_PART_BLOCK_STATES %d\n#define MIP_PART_SPLIT_STATES %d\n#define MIP_PART_QT_STATES 5\n"
             "#define MIP_PART_BLOCKS 16\n#define MIP_PART_NUM_LEVELS 6\n#define MIP_PART_LEVELS {%s}\n"
             % (len(st), t["nsplit"], ", ".join(str(v) for v in b)))
    o.append("typedef struct {\n  uint16_t cu0;\n  uint8_t shape, x, y, w, h, depth;\n} mip_part_state;\n")
    o.append("typedef struct {\n  uint16_t dx, dy[4], hi;\n} mip_part_step;\n")
    o.append("#define MIP_PART_STATE_TABLE { \\")
    for i in range(0, len(st), 4):
        o.append("  " + " ".join("{%4d,%2d,%2d,%2d,%2d,%2d,%d}," % (cu0, sh, x, y, w, h, d)
                                 for (x, y, w, h, d, cu0, sh) in st[i:i + 4]) + " \\")
    o.append("}\n")
    o.append("#define MIP_PART_CHILD_TABLE { \\")
    for row in t["child"]:
        o.append("  {" + ",".join("%5d" % c for c in row) + "}, \\")
    o.append("}\n")
    o.append("#define MIP_PART_QT_TABLE { \\")
    for row in t["qt"]:
        o.append("  {" + ",".join("%2d" % c for c in row) + "}, \\")
    o.append("}\n")
    o.append("/* per CU shape (zeros: the 64x64 shape and the _2half shapes head no state of the block) */")
    o.append("#define MIP_PART_STEP_TABLE { \\")
    for s in range(len(shapes())):
        dx, dy, hi = t["step"].get(s, (0, (0, 0, 0, 0), 0))
        o.append("  {%2d, {%4d,%4d,%4d,%4d}, %d}, \\" % (dx, *dy, hi))
    o.append("}\n")
    o.append("#endif")
    return "\n".join(o) + "\n"


if __name__ == "__main__":
    with open(DST, "w") as f:
        f.write(render())
    print("wrote", os.path.normpath(DST))
