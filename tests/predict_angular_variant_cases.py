"""Lists, selectors and expected blocks of the angular block-output tests -- a helper, not a test.

The default instance's suite (tests/test_gpu_predict_angular.py) and the suite of the three other
settings of (mip_angular_refs, mip_angular_interp) (tests/test_gpu_predict_angular_variants.py, with
its preconditions in tests/test_predict_angular_variants_cpu.py) draw the same lists from here, so
that the extended and the 4-tap kernels see what the default kernel sees.  Everything is computed
once and cached; callers do not modify what they get.

  variant   angular_refs   angular_interp   kernel                                     restatement
  ext2      EXTENDED       2TAP             angular_ext_predict_kernel                 angular_ext_ref
  sub4      SUBSTITUTED    4TAP             angular_tap4_predict_kernel, no table      angular_tap4_ref, lengths 0
  ext4      EXTENDED       4TAP             angular_tap4_predict_kernel, the table     angular_tap4_ref, real lengths
"""
from functools import lru_cache

import numpy as np

import angular_ext_cases as XC
import angular_ext_ref as X
import angular_ref as A
import angular_tap4_cases as TC
import angular_tap4_ref as T
import intra_cases as C
import intra_ref as I
import mipgpu
import oracle_lib as O
import predict_angular_caps as L
import predict_ref as P
import size_sweep as S
from mipgpu import layout

FILL = 0xABCD
PREFIX = np.cumsum([0] + [s.ncu for s in layout.SHAPES])
BASE = mipgpu.MODE_ANGULAR_BASE
ALL_CODES = BASE + np.arange(2, 67)
REGULAR = (I.MODE_PLANAR, I.MODE_DC)
PADDING = (-1, -1, -1, 0, 0)                                  # what mip_partition_device pads its list with

EXT, SUB = mipgpu.ANG_REFS_EXTENDED, mipgpu.ANG_REFS_SUBSTITUTED
TAP4, TAP2 = mipgpu.ANG_INTERP_4TAP, mipgpu.ANG_INTERP_2TAP
DEFAULT = "default"                                           # (SUB, TAP2): the setting of an engine nobody touched
VARIANTS = {"ext2": (EXT, TAP2), "sub4": (SUB, TAP4), "ext4": (EXT, TAP4)}
IDS = tuple(VARIANTS)
SETTINGS = (DEFAULT,) + IDS
SIZE = (264, 136)


def set_variant(eng, variant):
    """Puts the engine into the variant's setting; returns the engine."""
    eng.angular_refs, eng.angular_interp = VARIANTS[variant]
    return eng


# ---------------------------------------------------------------- expected blocks
def angular_blocks(refs, w, h, cus, modes=None):
    """{cu: uint16 [len(modes), bh, bw]} -- the blocks of angular_ref.predict on
    angular_ref.boundaries of refs [H, W] for the modes `modes` (None: all 65, slot m - 2)."""
    cus = np.asarray(cus, np.int64)
    shape, x, y, _, _ = layout.cu_geometry(w, h, cus)
    out = {}
    for s in layout.SHAPES:
        sel = np.nonzero(shape == s.index)[0]
        if sel.size:
            top, left, corner = A.boundaries(refs, x[sel], y[sel], s.w, s.h)
            blocks = A.predict(top, left, corner, s.w, s.h, modes).astype(np.uint16)
            for j, i in enumerate(sel):
                out[int(cus[i])] = blocks[:, j]
    return out


def regular_blocks(refs, w, h, cus):
    """{cu: uint16 [2, bh, bw]} -- Planar and DC from intra_ref.predict on predict_ref.boundaries."""
    cus = np.asarray(cus, np.int64)
    shape, x, y, _, _ = layout.cu_geometry(w, h, cus)
    out = {}
    for s in layout.SHAPES:
        sel = np.nonzero(shape == s.index)[0]
        if sel.size:
            b = [P.boundaries(refs, x[i], y[i], s.w, s.h)[:2] for i in sel]
            planar, dc = I.predict(np.stack([t for t, _ in b]), np.stack([l for _, l in b]), s.w, s.h)
            for j, i in enumerate(sel):
                out[int(cus[i])] = np.stack([planar[j], dc[j]]).astype(np.uint16)
    return out


def variant_lengths(variant, w, h, filt=None):
    """(E_top, E_left) per CU as the variant's kernel gets them: angular_ext_cases.lengths(w, h, filt)
    for the availability set of an engine with filter `filt` (None: the MIP_FILTER_NONE set, which
    is also what caller references go with), zeros for `sub4` and for the default setting."""
    _, e_top, e_left = XC.lengths(w, h, filt)
    if variant in (DEFAULT, "sub4"):
        return np.zeros_like(e_top), np.zeros_like(e_left)
    return e_top, e_left


def blocks(variant, refs, w, h, cus, modes=None, filt=None, clip=True):
    """{cu: uint16 [len(modes), bh, bw]} -- the blocks of the variant's restatement on refs [H, W]
    with the length set of `filt` (variant_lengths).  DEFAULT gives angular_blocks.  clip=False
    (4-tap variants only): int64 values before the clip."""
    if variant == DEFAULT:
        return angular_blocks(refs, w, h, cus, modes)
    cus = np.asarray(cus, np.int64)
    e_top, e_left = variant_lengths(variant, w, h, filt)
    shape, x, y, _, _ = layout.cu_geometry(w, h, cus)
    out = {}
    for s in layout.SHAPES:
        sel = np.nonzero(shape == s.index)[0]
        if sel.size:
            top, left, corner = X.boundaries(refs, x[sel], y[sel], s.w, s.h, e_top[cus[sel]], e_left[cus[sel]])
            if variant == "ext2":
                got = X.predict(top, left, corner, s.w, s.h, modes).astype(np.uint16)
            elif clip:
                got = T.predict(top, left, corner, s.w, s.h, modes).astype(np.uint16)
            else:
                got = T.predict(top, left, corner, s.w, s.h, modes, clip=False)
            for j, i in enumerate(sel):
                out[int(cus[i])] = got[:, j]
    return out


def block_of(variant, refs, x, y, bw, bh, e_top, e_left, mode):
    """One block [bh, bw] uint16 by the restatements' predict_cu (lengths as given)."""
    if variant == "ext2":
        return X.predict_cu(refs, x, y, bw, bh, e_top, e_left, mode)
    return T.predict_cu(refs, x, y, bw, bh, e_top, e_left, mode)


def used_length(w, h, cus, mode, e_top, e_left):
    """(E, S) per item: the extension of the item's main line -- E_top for the vertical class (mode
    >= 34), E_left for the horizontal one, as the table gives it -- and the side's length S, which
    is also the most an extension can be."""
    cus, mode = np.asarray(cus, np.int64), np.asarray(mode, np.int64)
    _, _, _, bw, bh = layout.cu_geometry(w, h, cus)
    vert = mode >= 34
    return np.where(vert, e_top[cus], e_left[cus]), np.where(vert, bh, bw)


def concat(want, cus, slots=None):
    """The packed output of a CU-major list: every CU's blocks (all of them, or the slots `slots`)
    back to back."""
    return np.concatenate([(want[int(c)] if slots is None else want[int(c)][slots]).reshape(-1) for c in cus])


# ---------------------------------------------------------------- 1. every shape, every mode
@lru_cache(maxsize=None)
def shape_case():
    """264x136, frame 1 of tests/intra_cases.py, the CU sample of tests/predict_ref.py and the
    default setting's blocks."""
    w, h = SIZE
    frame = C.frames(w, h, 2)[1]
    un = mipgpu.unavailable_cus(w, h)
    cus = P.sample_cus(w, h, un)
    return w, h, frame, un, cus, angular_blocks(frame, w, h, cus)


@lru_cache(maxsize=None)
def variant_shape_cus():
    """shape_case's CU sample plus angular_ext_cases.length_class_cus: sorted CU indexes at 264x136."""
    w, h, _, un, cus, _ = shape_case()
    _, e_top, e_left = XC.lengths(w, h, None)
    return np.union1d(cus, XC.length_class_cus(w, h, un, e_top, e_left))


@lru_cache(maxsize=None)
def shape_frames():
    """(frame 1, the 0 / 1023 frame) at 264x136."""
    w, h = SIZE
    f = C.frames(w, h, 3)
    return f[1], f[2]


@lru_cache(maxsize=None)
def shape_expected(setting, which):
    """The packed output of test 1 under `setting` (one of SETTINGS) on shape_frames()[which]:
    variant_shape_cus() CU-major, all 65 modes each."""
    w, h = SIZE
    cus = variant_shape_cus()
    out = concat(blocks(setting, shape_frames()[which], w, h, cus), cus)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- 2. the engine's own tables
TABLE_SHAPES = ("ALL_AL_64x64", "ALL_AL_4x32", "ALL_AL_32x4", "ALL_AL_16x16", "ALL_NA_8x32_G2", "ALL_AL_4x4")


def table_lists(w, h, filt):
    """[(shape, CU indexes)]: the largest shape, the most elongated ones and one of every size
    class, 8 CUs of the largest and 40 of every other, spread over the CUs available under `filt`."""
    nct = layout.num_ctus(w, h)
    un = mipgpu.unavailable_cus(w, h, filt).reshape(nct, layout.CUS_PER_CTU)
    lists = []
    for n in TABLE_SHAPES:
        s = layout.SHAPE_BY_NAME[n]
        ctu, c = np.nonzero(~un[:, PREFIX[s.index]:PREFIX[s.index + 1]])
        assert c.size
        k = ctu * layout.CUS_PER_CTU + PREFIX[s.index] + c
        lists.append((s, k[np.unique(np.linspace(0, k.size - 1, 8 if s.w == 64 else 40).astype(int))]))
    return lists


# source id -> (engine filter, frame of intra_cases.frames(w, h, 3), the references are the caller's)
TABLE_SOURCES = {"2d_int": (XC.FILTER_2D, 1, False), "1d_int": (C.FILTER, 2, False), "caller_refs": (XC.FILTER_2D, 0, True)}


@lru_cache(maxsize=None)
def table_source(source):
    """(engine filter, frame, references, the filter whose availability and length sets go with the
    references -- None for the caller's: the MIP_FILTER_NONE sets --, the other filter of the pair)."""
    w, h = SIZE
    filt, which, caller = TABLE_SOURCES[source]
    frame = C.frames(w, h, 3)[which]
    if caller:
        refs = S.caller_refs(w, h, 0)
        sets, other = None, filt
    else:
        refs = O.filter_frame(frame, filt, 0)
        sets, other = filt, None
    refs.setflags(write=False)
    return filt, frame, refs, sets, other


@lru_cache(maxsize=None)
def variant_table_lists(source):
    """table_lists of the source's right set, and with them every CU of those shapes, available in
    that set, whose lengths differ between the two sets of the pair -- the engine filter's, shortened
    by the filter's undefined samples, and the MIP_FILTER_NONE one: the spread sample alone holds
    none or one of them, and only they tell the engine's two length tables apart."""
    w, h = SIZE
    _, _, _, right, other = table_source(source)
    un, e_top, e_left = XC.lengths(w, h, right)
    _, o_top, o_left = XC.lengths(w, h, other)
    differ = ~un & ((e_top != o_top) | (e_left != o_left))
    shape = layout.cu_geometry(w, h, np.arange(un.size))[0]
    return [(s, np.union1d(k, np.nonzero(differ & (shape == s.index))[0])) for s, k in table_lists(w, h, right)]


@lru_cache(maxsize=None)
def table_expected(setting, source, sets="right"):
    """The packed output of test 2 under `setting` for `source`: variant_table_lists,
    shape-major, CU-major, all 65 modes.  sets="other": the same list with the lengths of the
    other set of the pair (what a swapped table index gives)."""
    w, h = SIZE
    _, _, refs, right, other = table_source(source)
    lists = variant_table_lists(source)
    out = np.concatenate([concat(blocks(setting, refs, w, h, k, None, right if sets == "right" else other), k) for _, k in lists])
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def table_restatement(variant, source):
    """The restatement's tables {cost, sad, satd} [nCTUs*5380, 65] for the one frame of `source`."""
    w, h = SIZE
    _, frame, refs, sets, _ = table_source(source)
    un = mipgpu.unavailable_cus(w, h, sets)
    e_top, e_left = variant_lengths(variant, w, h, sets)
    tabs = (X if variant == "ext2" else T).tables(frame, refs, un, e_top, e_left)
    for v in tabs.values():
        v.setflags(write=False)
    return tabs


# ---------------------------------------------------------------- 3. mixed quads and the flag matrix
ANG_KINDS = {"ang_h+": 6, "ang_h-": 27, "ang_v-": 41, "ang_v+": 60, "ang_18": 18, "ang_50": 50}
PER_BAD_KIND = 12
BAD_KINDS = ("unavailable", "pitch_low", "pitch_2", "offset_2", "frame", "mode_80", "mode_81", "mode_c3", "mode_ff")


@lru_cache(maxsize=None)
def mixed_case(w=136, h=72, seed=0x4A):
    """(w, h, frame, un, cus, kind, cu, items, total): MIP, Planar, DC, six angular kinds and nine
    kinds of rejected entry over a one-per-shape CU sample, shuffled so that every kind stands in
    every quad position, and a last angular item one sample too long for `out`."""
    frame = C.case(w, h, None)[0][1]
    un = mipgpu.unavailable_cus(w, h)
    assert [A.ANGLE[ANG_KINDS[k]] for k in ("ang_h+", "ang_h-", "ang_v-", "ang_v+")] == [20, -14, -14, 16]
    assert [ANG_KINDS[k] < 34 for k in ("ang_h+", "ang_h-", "ang_v-", "ang_v+")] == [True, True, False, False]
    rng = np.random.default_rng(seed)
    cus = P.sample_cus(w, h, un, seed=seed, per_shape=1)
    shape, _, _, bw, bh = layout.cu_geometry(w, h, cus)
    small = bw * bh <= 64
    assert small.any() and (~small).any()
    good = ["mip", "planar", "dc"] + list(ANG_KINDS)
    kind, cu = [], []
    for k in good:
        kind += [k] * cus.size
        cu += list(cus)
    wide = cus[bw >= 16]
    for k in BAD_KINDS:
        for j in range(PER_BAD_KIND):
            kind.append(k)
            cu.append(int(rng.choice(np.nonzero(un)[0]) if k == "unavailable" else rng.choice(wide) if k == "pitch_low" else rng.choice(cus)))
    kind, cu = np.array(kind), np.array(cu, np.int64)
    for shuffle in range(256):                                # a shuffle that puts every kind into every quad position
        order = np.random.default_rng(shuffle).permutation(cu.size)
        if all(set(kind[order][p::4]) == set(kind) for p in range(4)):
            break
    else:
        raise AssertionError("no shuffle mixes the kinds over the quad positions")
    kind, cu = kind[order], cu[order]
    last = layout.cu_geometry(w, h, cus)[3].argmax()          # the list ends with a large angular item that is
    kind, cu = np.append(kind, "past_end"), np.append(cu, cus[last])   # one sample too long for `out`
    gshape = layout.cu_geometry(w, h, cu)[0]
    mode = np.zeros(cu.size, np.int64)
    for i, k in enumerate(kind):
        if k == "mip":
            mode[i] = rng.integers(0, layout.SHAPES[gshape[i]].total_modes)
        elif k in ("planar", "dc"):
            mode[i] = REGULAR[k == "dc"]
        elif k in ANG_KINDS:
            mode[i] = BASE + ANG_KINDS[k]
        else:                                                 # rejected entries carry every kind of valid mode
            mode[i] = (BASE + 34, BASE + 2, REGULAR[0], 1)[i % 4] if k != "past_end" else BASE + 23
    items, total = mipgpu.pred_items(w, h, 0, cu, mode)
    items["pitch"][kind == "pitch_low"] = 8
    items["pitch"][kind == "pitch_2"] += 2
    items["offset"][kind == "offset_2"] += 2
    items["frame"][kind == "frame"] = 1                       # == nframes of the call
    for k, code in (("mode_80", 0x80), ("mode_81", 0x81), ("mode_c3", 0xC3), ("mode_ff", 0xFF)):
        items["mode"][kind == k] = code
    return w, h, frame, un, cus, kind, cu, items, total


def wave_groups(accepted, small):
    """The groups of up to four small items that the angular kernels hand to the four 16-lane groups
    of a wave in one step: per row of 64 list entries, the accepted small items in entry order, four
    at a time (the last group of a row may hold fewer).  `accepted` and `small` are bool per entry;
    returns a list of index arrays."""
    groups = []
    accepted, small = np.asarray(accepted, bool), np.asarray(small, bool)
    for r0 in range(0, accepted.size, L.ENTRIES_PER_WAVE):
        at = r0 + np.nonzero((accepted & small)[r0:r0 + L.ENTRIES_PER_WAVE])[0]
        groups += [at[q:q + 4] for q in range(0, at.size, 4)]
    return groups


def four_length_groups(w, h, kind, cu, e_top, e_left):
    """The wave_groups of a mixed_case list that hold four items of four different (E_top, E_left)
    pairs, both classes, and four different used lengths (the E each item's own main line takes)."""
    _, _, _, gw, gh = layout.cu_geometry(w, h, cu)
    accepted = np.isin(kind, list(ANG_KINDS))
    mode = np.array([ANG_KINDS.get(k, 0) for k in kind])
    used = np.where(mode >= 34, e_top[cu], e_left[cu])
    hits = []
    for g in wave_groups(accepted, gw * gh <= 64):
        if g.size == 4 and len({(int(e_top[cu[i]]), int(e_left[cu[i]])) for i in g}) == 4 and \
                len(set(mode[g] >= 34)) == 2 and len(set(used[g])) == 4:
            hits.append(g)
    return hits


MIXED_VARIANT_SEED = 0x4B      # the first seed from the default list's 0x4A on whose 136x72 sample has a four_length_groups group


def mixed_variant_case():
    """The mixed_case of the variants' flag matrix."""
    return mixed_case(136, 72, MIXED_VARIANT_SEED)


def mixed_expected(case, setting, flags):
    """(the 2 * total samples a call with `flags` leaves in a FILL-ed tensor, its skipped count) for
    a mixed_case tuple, the angular items taken from `setting`'s restatement."""
    w, h, frame, un, cus, kind, cu, items, total = case
    gshape, x, y, gw, gh = layout.cu_geometry(w, h, cu)
    table_modes = tuple(sorted(ANG_KINDS.values()))
    ang_want = blocks(setting, frame, w, h, cus, table_modes)
    slot = {m: i for i, m in enumerate(table_modes)}
    reg_want = regular_blocks(frame, w, h, cus)
    out = np.full(2 * total, FILL, np.uint16)
    written = 0
    for i, it in enumerate(items):
        k = kind[i]
        if k == "mip":
            blk = P.CuPredictor(frame, x[i], y[i], gshape[i]).predict(int(it["mode"]))
        elif k in ("planar", "dc") and flags & mipgpu.PRED_REGULAR:
            blk = reg_want[int(cu[i])][int(k == "dc")]
        elif k in ANG_KINDS and flags & mipgpu.PRED_ANGULAR:
            blk = ang_want[int(cu[i])][slot[ANG_KINDS[k]]]
        else:
            continue
        out[it["offset"]:it["offset"] + gw[i] * gh[i]] = blk.reshape(-1)
        written += 1
    return out, items.size - written


# ---------------------------------------------------------------- 4. narrow stores and unaligned rows
NARROW_SIZES = ((132, 136), (260, 72))


@lru_cache(maxsize=None)
def narrow_case(w, h):
    """(frame, cus, shape, x, y, bw, bh, modes, used): a set of CUs of mixed shapes that do not
    overlap, wholly inside the frame, with the modes cycling through all 65; used [H, W] marks
    their samples."""
    frame = C.frames(w, h, 2)[1]
    un = mipgpu.unavailable_cus(w, h)
    cand = P.sample_cus(w, h, un, seed=w, per_shape=10)
    cand = cand[np.random.default_rng(w).permutation(cand.size)]
    shape, x, y, bw, bh = layout.cu_geometry(w, h, cand)
    used, keep = np.zeros((h, w), bool), []
    for i in range(cand.size):
        if x[i] + bw[i] <= w and not used[y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]].any():
            used[y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] = True
            keep.append(i)
    keep = np.array(keep)
    cus, shape, x, y, bw, bh = cand[keep], shape[keep], x[keep], y[keep], bw[keep], bh[keep]
    modes = 2 + (np.arange(cus.size) * 7) % 65
    return frame, cus, shape, x, y, bw, bh, modes, used


@lru_cache(maxsize=None)
def four_wide_case():
    """(w, h, frame, cus, bh, modes): the 4-wide CUs (4x4 to 4x32) of a four-per-shape sample at
    136x72, modes cycling."""
    w, h = 136, 72
    frame = C.case(w, h, None)[0][2]
    un = mipgpu.unavailable_cus(w, h)
    cus = P.sample_cus(w, h, un, seed=0x77, per_shape=4)
    shape, x, y, bw, bh = layout.cu_geometry(w, h, cus)
    cus, bh = cus[bw == 4], bh[bw == 4]
    modes = 2 + (np.arange(cus.size) * 11) % 65
    return w, h, frame, cus, bh, modes


# ---------------------------------------------------------------- 5. multi-pass
MULTIPASS_MODES = (2, 18, 29, 34, 45, 50, 66)


@lru_cache(maxsize=None)
def multipass_list(seed=0x6D):
    """The 611 669-entry list of the multi-pass tests at 136x72, as a dict: mostly partition padding,
    one angular item per 64-entry row, seven in every 97th row, 3000 MIP / Planar items elsewhere,
    the last entry (in a partial row) an angular item.  `seed` draws the CU pool (24 small CUs, 8
    of 65..512 samples) and the items.  Keys: w h frame n rows cus shape x y bw bh (the pool) ang_pos
    per_row at which kind slot mode (the real entries: kind 0 angular, 1 MIP mode 0, 2 Planar; slot
    into MULTIPASS_MODES) real (their items) total items (the whole list)."""
    w, h = 136, 72
    frame = C.case(w, h, None)[0][0]
    un = mipgpu.unavailable_cus(w, h)
    n = L.multipass_work(L.ENTRIES_PER_ROUND)
    rows = -(-n // L.ENTRIES_PER_WAVE)
    rng = np.random.default_rng(seed)
    cus = P.sample_cus(w, h, un, seed=seed, per_shape=1)
    shape, x, y, bw, bh = layout.cu_geometry(w, h, cus)
    pick = np.concatenate([rng.choice(np.nonzero(bw * bh <= 64)[0], 24), rng.choice(np.nonzero((bw * bh > 64) & (bw * bh <= 512))[0], 8)])
    cus, shape, x, y, bw, bh = cus[pick], shape[pick], x[pick], y[pick], bw[pick], bh[pick]
    # positions: one angular item per row, six more in every 97th row, the last entry; then MIP / Planar items elsewhere
    pos = np.arange(rows) * L.ENTRIES_PER_WAVE + (np.arange(rows) * 7) % L.ENTRIES_PER_WAVE
    pos[-1] = n - 1
    busy = np.arange(0, rows - 1, 97)
    extra = (busy[:, None] * L.ENTRIES_PER_WAVE + (busy[:, None] * 7 + 1 + 9 * np.arange(6)[None, :]) % L.ENTRIES_PER_WAVE).reshape(-1)
    ang_pos = np.unique(np.concatenate([pos, extra]))
    per_row = np.bincount(ang_pos // L.ENTRIES_PER_WAVE, minlength=rows)
    free = np.setdiff1d(np.arange(n), ang_pos)
    other_pos = rng.choice(free, 3000, replace=False)
    at = np.concatenate([ang_pos, other_pos])
    order = np.argsort(at)
    which = rng.integers(0, cus.size, at.size)
    kind = np.concatenate([np.zeros(ang_pos.size, int), rng.integers(1, 3, other_pos.size)])   # 0 angular, 1 MIP, 2 Planar
    slot = rng.integers(0, len(MULTIPASS_MODES), at.size)
    mode = np.where(kind == 0, BASE + np.array(MULTIPASS_MODES)[slot], np.where(kind == 1, 0, I.MODE_PLANAR))
    at, which, kind, slot, mode = at[order], which[order], kind[order], slot[order], mode[order]
    real, total = mipgpu.pred_items(w, h, 0, cus[which], mode)
    items = np.zeros(n, mipgpu.PRED_ITEM)
    items[:] = PADDING
    items[at] = real
    return dict(w=w, h=h, frame=frame, n=n, rows=rows, cus=cus, shape=shape, x=x, y=y, bw=bw, bh=bh, busy=busy, ang_pos=ang_pos,
                per_row=per_row, at=at, which=which, kind=kind, slot=slot, mode=mode, real=real, total=total, items=items)


def multipass_expected(m, setting):
    """The total + 64 samples the multi-pass list leaves in a FILL-ed tensor with flags 5, the
    angular items from `setting`'s restatement."""
    w, h, frame, cus = m["w"], m["h"], m["frame"], m["cus"]
    ang_want = blocks(setting, frame, w, h, cus, MULTIPASS_MODES)
    reg_want = regular_blocks(frame, w, h, cus)
    expect = np.full(m["total"] + 64, FILL, np.uint16)
    mip = {i: P.CuPredictor(frame, m["x"][i], m["y"][i], m["shape"][i]).predict(0) for i in range(cus.size)}
    which, kind, slot, real = m["which"], m["kind"], m["slot"], m["real"]
    for i in range(m["at"].size):
        c = which[i]
        blk = ang_want[int(cus[c])][slot[i]] if kind[i] == 0 else mip[c] if kind[i] == 1 else reg_want[int(cus[c])][0]
        expect[real["offset"][i]:real["offset"][i] + m["bw"][c] * m["bh"][c]] = blk.reshape(-1)
    return expect


def extension_changes(m, e_top, e_left):
    """The (row r, row r + ROWS_PER_ROUND) pairs of consecutive passes of one wave in which each row
    holds exactly one angular item, both go to the same LDS words (both small: group 0; both large:
    the wave's) with the same S and M -- the first one's extension words are the words right behind
    the second one's line, where a read that is not clamped lands --, the first one's main line has
    its full extension E = S >= 8 and the second one, of a mode with a positive angle (2 or 66: it
    reads up to the line's end), has none."""
    w, h = m["w"], m["h"]
    ang = m["kind"] == 0
    at, cu, mode = m["at"][ang], m["cus"][m["which"][ang]], m["mode"][ang] - BASE
    used, side = used_length(w, h, cu, mode, e_top, e_left)
    _, _, _, bw, bh = layout.cu_geometry(w, h, cu)
    main = np.where(mode >= 34, bw, bh)
    small = (m["bw"] * m["bh"] <= 64)[m["which"][ang]]
    row = at // L.ENTRIES_PER_WAVE
    single = m["per_row"] == 1
    first = {int(r): i for i, r in enumerate(row) if single[r]}
    hits = []
    for r, i in first.items():
        j = first.get(r + L.ROWS_PER_ROUND)
        if j is not None and small[i] == small[j] and side[i] == side[j] and main[i] == main[j] and used[i] == side[i] >= 8 and used[j] == 0 and mode[j] in (2, 66):
            hits.append((r, r + L.ROWS_PER_ROUND))
    return hits


MULTIPASS_VARIANT_SEED = 0x78   # of the pool seeds 0x6D .. 0x84 the one with the most extension_changes pairs (43; the default's 0x6D: 1)


def multipass_variant_list():
    """The multipass_list of the variants' scan."""
    return multipass_list(MULTIPASS_VARIANT_SEED)


# ---------------------------------------------------------------- 6. frame edges
EDGE_SIZES = tuple(S.ALL_SIZES[::5])


def room(w, h, cus):
    """(top, left) per CU: how many samples of row y - 1 lie right of the CU inside the frame, and how
    many of column x - 1 below it (0 without that row / column): what the kernels cut E to."""
    _, x, y, bw, bh = layout.cu_geometry(w, h, cus)
    return np.where(y > 0, np.maximum(w - (x + bw), 0), 0), np.where(x > 0, np.maximum(h - (y + bh), 0), 0)


def sizes_where_the_table_exceeds_the_room():
    """The sizes of tests/size_sweep.py at which some available CU's E_top or E_left is larger than
    room() -- where the kernels' cut does something."""
    hits = []
    for w, h in S.ALL_SIZES:
        un, e_top, e_left = XC.lengths(w, h, None)
        k = np.nonzero(~un)[0]
        rt, rl = room(w, h, k)
        if (e_top[k] > rt).any() or (e_left[k] > rl).any():
            hits.append((w, h))
    return hits


@lru_cache(maxsize=None)
def edge_case(w, h):
    """(noise frame of tests/size_sweep.py, availability set, CUs np.nonzero(~un)[0][::37], their
    modes: angular_tap4_cases.SWEEP_LIST cycling)."""
    frame = S.content("noise", w, h)
    un = mipgpu.unavailable_cus(w, h)
    cus = np.nonzero(~un)[0][::37]
    modes = np.array(TC.SWEEP_LIST)[np.arange(cus.size) % len(TC.SWEEP_LIST)]
    return frame, un, cus, modes

