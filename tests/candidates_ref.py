"""K-best candidate lists over MIP, Planar / DC and angular modes -- a numpy restatement of
mip_candidates_device written from the text of include/mipgpu.h (a helper, not a test; pinned by
tests/test_candidates_cpu.py).

Per CU a row of 99 columns, one per rank: column v is MIP mode v (0..31), 32 Planar, 33 DC,
32 + m angular mode m (34..98).  A column holds the candidate's value (cost + bias), or ABSENT.
A stable sort of the row is the order by (value, rank); the first k columns are the list, entries
that land on an ABSENT column are 0xff / UNAVAILABLE."""
import numpy as np

UN = 0x7FFFFFFF                 # MIP_COST_UNAVAILABLE
ABSENT = np.int64(1) << 40      # above every value
RANKS = 99
CODE = np.array(list(range(32)) + [0xF0, 0xF1] + [0x80 + m for m in range(2, 67)], np.uint8)   # rank -> mode code
MAX_K, MAX_BIAS = 32, 1 << 20
TOP = (1 << 24) - 1 - (1 << 20)  # the largest table value of the domain


def rows(ncu, mip_mode=None, mip_cost=None, intra_cost=None, intra_bias=None, ang_cost=None, ang_bias=0):
    """int64 [ncu, 99]: every CU's candidate values by rank.  Inputs are [ncu, kin], [ncu, 2], [ncu, 65]."""
    v = np.full((ncu, RANKS), ABSENT, np.int64)
    if mip_mode is not None:
        mode, cost = np.asarray(mip_mode).reshape(ncu, -1).astype(np.int64), np.asarray(mip_cost).reshape(ncu, -1).astype(np.int64)
        for r in range(mode.shape[1]):
            ok = (mode[:, r] <= 31) & (cost[:, r] != UN)
            v[np.nonzero(ok)[0], mode[ok, r]] = cost[ok, r]
    if intra_cost is not None:
        c = np.asarray(intra_cost).reshape(ncu, 2).astype(np.int64)
        bias = np.zeros(2, np.int64) if intra_bias is None else np.asarray(intra_bias, np.int64)
        v[:, 32:34] = np.where(c != UN, c + bias, ABSENT)
    if ang_cost is not None:
        c = np.asarray(ang_cost).reshape(ncu, 65).astype(np.int64)
        v[:, 34:99] = np.where(c != UN, c + int(ang_bias), ABSENT)
    return v


def candidates(k, mip_mode=None, mip_cost=None, intra_cost=None, intra_bias=None, ang_cost=None, ang_bias=0):
    """(modes uint8, costs int32), each [..., k], for inputs of shape [..., kin] / [..., 2] / [..., 65]."""
    assert 1 <= k <= MAX_K
    first = next(a for a in (mip_mode, intra_cost, ang_cost) if a is not None)
    lead = np.asarray(first).shape[:-1]
    ncu = int(np.prod(lead))
    v = rows(ncu, mip_mode, mip_cost, intra_cost, intra_bias, ang_cost, ang_bias)
    order = np.argsort(v, axis=1, kind="stable")[:, :k]       # ties: the lower rank first
    value = np.take_along_axis(v, order, axis=1)
    none = value == ABSENT
    modes = np.where(none, 0xFF, CODE[order]).astype(np.uint8)
    costs = np.where(none, UN, value).astype(np.int32)
    return modes.reshape(lead + (k,)), costs.reshape(lead + (k,))


def count(mip_mode=None, mip_cost=None, intra_cost=None, ang_cost=None):
    """Candidates per CU, [...]."""
    first = next(a for a in (mip_mode, intra_cost, ang_cost) if a is not None)
    lead = np.asarray(first).shape[:-1]
    v = rows(int(np.prod(lead)), mip_mode, mip_cost, intra_cost, None, ang_cost, 0)
    return (v != ABSENT).sum(axis=1).reshape(lead)


def top_of_domain(ncu, seed):
    """Tables of 0, 8 380 416 (the engine's largest cost) and TOP, three MIP entries and about 21
    candidates per CU, so that lists of 32 reach the largest values; for biases of MAX_BIAS."""
    rng = np.random.default_rng(seed)
    values = np.array([0, 0, 8380416, TOP], np.int32)
    ang = rng.choice(values, (ncu, 65))
    ang[rng.random((ncu, 65)) < 0.75] = UN
    return {"mip_mode": np.argsort(rng.random((ncu, 32)), axis=1)[:, :3].astype(np.uint8), "mip_cost": rng.choice(values, (ncu, 3)),
            "intra_cost": rng.choice(values, (ncu, 2)), "ang_cost": ang}


def synthetic(ncu, kin, seed, high=8):
    """Tables where ties are the rule: costs in 0..high-1; about 5 % of the CUs UNAVAILABLE in every
    family; about 10 % with one family alive; MIP lists of distinct modes, with 0xff tails (entries
    past a random length are 0xff / UNAVAILABLE) and a few modes above 31 (absent by rule, with
    ordinary costs)."""
    rng = np.random.default_rng(seed)
    mip_cost = rng.integers(0, high, (ncu, kin)).astype(np.int32)
    mip_mode = np.argsort(rng.random((ncu, 32)), axis=1)[:, :kin].astype(np.uint8)     # distinct modes per CU
    length = rng.integers(0, kin + 1, ncu)
    tail = np.arange(kin)[None, :] >= length[:, None]
    mip_mode[tail], mip_cost[tail] = 0xFF, UN
    above = (rng.random((ncu, kin)) < 0.03) & ~tail
    mip_mode[above] = rng.integers(32, 255, int(above.sum())).astype(np.uint8)
    intra = rng.integers(0, high, (ncu, 2)).astype(np.int32)
    ang = rng.integers(0, high, (ncu, 65)).astype(np.int32)
    ang[rng.random((ncu, 65)) < 0.5] = UN                     # unlisted / unevaluated slots
    dead = rng.random(ncu) < 0.05
    only = np.where(rng.random(ncu) < 0.10, rng.integers(0, 3, ncu), -1)              # the one family alive
    off = dead[:, None] | ((only >= 0) & (only != 0))[:, None]
    mip_mode[np.broadcast_to(off, mip_mode.shape)], mip_cost[np.broadcast_to(off, mip_cost.shape)] = 0xFF, UN
    intra[dead | ((only >= 0) & (only != 1))] = UN
    ang[dead | ((only >= 0) & (only != 2))] = UN
    return {"mip_mode": mip_mode, "mip_cost": mip_cost, "intra_cost": intra, "ang_cost": ang}
