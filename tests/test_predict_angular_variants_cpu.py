"""Preconditions of tests/test_gpu_predict_angular_variants.py (no GPU): on the numpy restatements
and the lists of tests/predict_angular_variant_cases.py alone, before any launch -- the lists tell
the four block-output settings and the engine's two length tables apart, they reach every shape,
mode, length class and interpolation table, the cubic leaves the 10-bit range on both sides, the
mixed list puts four different extensions into one step of a wave, the multi-pass list changes the
extension between the passes of a wave, and the frame-edge `room` cut has nothing to do."""
import itertools

import numpy as np

import angular_ext_cases as XC
import angular_tap4_ref as T
import mipgpu
import predict_angular_caps as L
import predict_angular_variant_cases as V
from mipgpu import layout


def _differing(a, b):
    assert a.size == b.size
    return int((a != b).sum())


# ---------------------------------------------------------------- pairwise differences
def test_the_settings_expected_outputs_differ_pairwise_on_the_shape_list():
    """Test 1's list, 16 495 440 samples: any two of the four settings differ in more than 2 % of
    them.  Fewest on frame 1: default / ext2 808 094 and sub4 / ext4 981 524 (the extension alone);
    on the 0 / 1023 frame: 453 972 and 569 465; a 2-tap against a 4-tap setting 4.8 to 12.4 million
    -- a launch of another setting's kernel cannot pass."""
    for which in (0, 1):
        for a, b in itertools.combinations(V.SETTINGS, 2):
            n = _differing(V.shape_expected(a, which), V.shape_expected(b, which))
            print("shape list, frame %d, %s / %s: %d of %d samples differ" % (which, a, b, n, V.shape_expected(a, which).size))
            assert n > 0.02 * V.shape_expected(a, which).size, (which, a, b)


def test_the_settings_and_the_two_length_sets_differ_on_the_table_lists():
    """Test 2's lists (4.2 million samples per source): any two settings differ in more than 100 000
    samples per source (fewest: default / ext2 at 1d_int, 171 448), and under ext2 / ext4 the filter's length set and the MIP_FILTER_NONE set
    differ in 3 234 .. 6 470 samples (2d_int 3 234 / 3 675, 1d_int 4 303 / 4 891, caller_refs 4 762 /
    6 470), in the 18 / 39 / 33 CUs whose lengths differ, nearly all of which variant_table_lists adds -- a swapped table index cannot pass.
    sub4 takes no table."""
    w, h = V.SIZE
    for source in V.TABLE_SOURCES:
        for a, b in itertools.combinations(V.SETTINGS, 2):
            n = _differing(V.table_expected(a, source), V.table_expected(b, source))
            print("table list, %s, %s / %s: %d samples differ" % (source, a, b, n))
            assert n > 100000, (source, a, b)
        _, _, _, right, other = V.table_source(source)
        assert (right is None) != (other is None)
        for variant in ("ext2", "ext4"):
            n = _differing(V.table_expected(variant, source), V.table_expected(variant, source, "other"))
            print("table list, %s, %s: %d samples differ between the two length sets" % (source, variant, n))
            assert n >= 3000, (source, variant)
        assert np.array_equal(V.table_expected("sub4", source), V.table_expected("sub4", source, "other"))
        # the lists hold the default test's six shapes, all CUs available in the source's set, CUs of both tables' kinds
        un, e_top, e_left = XC.lengths(w, h, right)
        _, o_top, o_left = XC.lengths(w, h, other)
        lists = V.variant_table_lists(source)
        assert [s.name for s, _ in lists] == list(V.TABLE_SHAPES)
        k = np.concatenate([k for _, k in lists])
        assert not un[k].any() and np.unique(k).size == k.size
        differ = (e_top[k] != o_top[k]) | (e_left[k] != o_left[k])
        print("table list, %s: %d of %d CUs have other lengths in the other set" % (source, differ.sum(), k.size))
        assert differ.sum() >= 18 and (~differ).sum() >= 200


# ---------------------------------------------------------------- test 1
def test_shape_list_coverage():
    """Test 1's 1 280 CUs at 264x136: every shape (and so, with all 65 modes each, every (shape,
    mode) pair); no, a partial and the full extension on the top line (864 / 135 / 281 CUs) and on
    the left line (939 / 142 / 199); in every size class (lw + lh) >> 1 that has cubic and Gaussian
    modes both occur, and mip_angular_filter is the restatement's choice."""
    w, h, _, un, sample, _ = V.shape_case()
    cus = V.variant_shape_cus()
    _, e_top, e_left = XC.lengths(w, h, None)
    shape, x, y, bw, bh = layout.cu_geometry(w, h, cus)
    assert not un[cus].any() and np.isin(sample, cus).all() and cus.size > sample.size
    assert set(shape) == set(range(layout.NUM_SHAPES))
    kt, kl = XC.length_class(e_top[cus], bh), XC.length_class(e_left[cus], bw)
    print("top line: none / partial / full", np.bincount(kt, minlength=3), "left line:", np.bincount(kl, minlength=3))
    assert np.bincount(kt, minlength=3).min() >= 90 and np.bincount(kl, minlength=3).min() >= 90
    for s in layout.SHAPES:                                    # per shape: the classes that exist among its available CUs are in the list
        every = np.nonzero(~un & (layout.cu_geometry(w, h, np.arange(un.size))[0] == s.index))[0]
        for e, full, line in ((e_top, s.h, kt), (e_left, s.w, kl)):
            assert set(XC.length_class(e[every], full)) == set(line[shape == s.index]), s.name
    classes = {}
    for s in layout.SHAPES:
        lw, lh = s.w.bit_length() - 1, s.h.bit_length() - 1
        tables = {mipgpu.angular_filter(lw, lh, m) for m in range(2, 67)}
        assert all(mipgpu.angular_filter(lw, lh, m) == int(T.filter_gauss(lw, lh, m)) for m in range(2, 67)), s.name
        classes.setdefault((lw + lh) >> 1, set()).update(tables)
    print("interpolation tables per size class:", classes)
    assert all(t == {0, 1} for c, t in classes.items() if c >= 3) and classes[2] == {0}      # 4x4, 4x8, 8x4: cubic only
    assert len(classes) >= 4


OVERSHOOT = {"sub4": (559828, 579246), "ext4": (594688, 619751)}         # measured on the restatement: samples (below 0, above 1023)


def test_the_cubic_overshoots_on_the_0_1023_frame():
    """Before the clip (angular_tap4_ref.predict(clip=False)) the 4-tap samples of test 1's list lie
    below 0 in 559 828 (sub4, 3.394 %) / 594 688 (ext4, 3.605 %) of the 16 495 440 samples on the
    0 / 1023 frame and above 1023 in 579 246 (3.512 %) / 619 751 (3.757 %): OVERSHOOT.  Each count is
    asserted at no less than half of its own figure.  (On frame 1: 0.23 % on either side.)"""
    w, h = V.SIZE
    cus = V.variant_shape_cus()
    for variant in ("sub4", "ext4"):
        raw = V.blocks(variant, V.shape_frames()[1], w, h, cus, clip=False)
        n = sum(b.size for b in raw.values())
        below = sum(int((b < 0).sum()) for b in raw.values())
        above = sum(int((b > 1023).sum()) for b in raw.values())
        print("%s on the 0 / 1023 frame: %d below 0, %d above 1023 of %d samples" % (variant, below, above, n))
        assert n == 16495440 and 2 * below >= OVERSHOOT[variant][0] and 2 * above >= OVERSHOOT[variant][1], variant
        clipped = V.shape_expected(variant, 1)
        assert clipped.min() == 0 and clipped.max() == 1023


# ---------------------------------------------------------------- test 3
def test_mixed_list_quads():
    """The variants' mixed list (136x72, sample seed 0x4B, 1 315 entries): every kind and both block
    sizes in every quad position, angular items next to MIP, Planar / DC and rejected ones, as the
    default setting's test asserts of its list; and 2 steps of a wave hand its four 16-lane groups
    four small angular items of four different (E_top, E_left) pairs, of both classes, whose own main
    lines take four different extensions: (0, 8) (12, 0) (4, 0) (0, 0)."""
    w, h, frame, un, cus, kind, cu, items, total = V.mixed_variant_case()
    n = items.size
    _, x, y, gw, gh = layout.cu_geometry(w, h, cu)
    is_ang = np.isin(kind, list(V.ANG_KINDS))
    assert items["offset"][-1] + gw[-1] * gh[-1] == total and kind[-1] == "past_end"
    for p in range(4):
        at = np.arange(p, n, 4)
        assert {"mip", "planar", "dc"} <= set(kind[at]) and set(V.ANG_KINDS) <= set(kind[at]) and set(V.BAD_KINDS) <= set(kind[at]), p
        a = at[is_ang[at]]
        assert (gw[a] * gh[a] <= 64).any() and (gw[a] * gh[a] > 64).any(), p
    quads = [set(kind[q:q + 4]) for q in range(0, n - 3, 4)]
    assert any(q & set(V.ANG_KINDS) and "mip" in q for q in quads) and any(q & set(V.ANG_KINDS) and q & {"planar", "dc"} for q in quads)
    assert any(q & set(V.ANG_KINDS) and q & set(V.BAD_KINDS) for q in quads)
    _, e_top, e_left = XC.lengths(w, h, None)
    hits = V.four_length_groups(w, h, kind, cu, e_top, e_left)
    print("groups of four different lengths:", [[(str(kind[i]), int(e_top[cu[i]]), int(e_left[cu[i]])) for i in g] for g in hits])
    assert len(hits) >= 2
    for g in hits:                                            # between them: entries the kernel leaves alone
        assert g.max() // L.ENTRIES_PER_WAVE == g.min() // L.ENTRIES_PER_WAVE
    assert any(not is_ang[g.min():g.max() + 1].all() for g in hits)
    # the default setting's list is the one it was
    assert V.mixed_case()[4].size and V.mixed_case() is not V.mixed_variant_case()


# ---------------------------------------------------------------- test 5
def test_multipass_list_passes_and_extension_change():
    """The variants' multi-pass list (pool seed 0x78): 611 669 entries, 9 558 rows, every wave emits
    in each of its two or three passes, rows of one and of seven angular items, small and large
    blocks, as the default setting's test asserts of its list; and in 43 pairs of consecutive passes
    of one wave the first pass's only item has its full extension (E = S >= 8) and the second pass's
    only item, in the same LDS words, with the same S and M and of a mode that reads up to its line's
    end, has none -- the first one's extension words lie right behind the second one's line."""
    m = V.multipass_variant_list()
    n, rows, per_row, ang_pos, busy, at, kind, which = (m[k] for k in ("n", "rows", "per_row", "ang_pos", "busy", "at", "kind", "which"))
    assert n == L.multipass_work(L.ENTRIES_PER_ROUND) == 611669 and rows == -(-n // L.ENTRIES_PER_WAVE)
    assert n < 1 << 20 and n % L.ENTRIES_PER_WAVE and L.passes(rows, L.ROWS_PER_ROUND) == (2, 3)
    assert ang_pos.max() == n - 1 and ang_pos.size == rows + busy.size * 6
    assert per_row.min() >= 1 and per_row.max() == 7
    wave = np.arange(rows) % L.ROWS_PER_ROUND
    assert np.bincount(wave, weights=per_row > 0, minlength=L.ROWS_PER_ROUND).min() >= 2
    small = (m["bw"] * m["bh"] <= 64)[which]
    assert (small & (kind == 0)).any() and (~small & (kind == 0)).any() and at.size < n // 20
    assert (kind == 1).any() and (kind == 2).any()
    _, e_top, e_left = XC.lengths(m["w"], m["h"], None)
    hits = V.extension_changes(m, e_top, e_left)
    print("extension changes between passes:", len(hits), hits[:4])
    assert len(hits) >= 40 and all(b - a == L.ROWS_PER_ROUND for a, b in hits)
    used, _ = V.used_length(m["w"], m["h"], m["cus"][which[kind == 0]], m["mode"][kind == 0] - V.BASE, e_top, e_left)
    assert (used > 0).mean() > 0.1                            # the extension is no rarity in the list


# ---------------------------------------------------------------- test 6
def test_no_table_length_exceeds_the_room():
    """At none of the 70 sizes of tests/size_sweep.py does an available CU's E_top exceed the samples
    left in row y - 1 right of it, or its E_left those of column x - 1 below it: the rule behind the
    table already stops at the frame's edge, so the kernels' `room` cut changes nothing the engine's
    own table gives, and test 6 has no further sizes.  The sizes it runs do have extensions that end
    at the right and the bottom edge (E == room > 0)."""
    assert V.sizes_where_the_table_exceeds_the_room() == []
    ends = 0
    for w, h in V.EDGE_SIZES:
        frame, un, cus, modes = V.edge_case(w, h)
        _, e_top, e_left = XC.lengths(w, h, None)
        rt, rl = V.room(w, h, cus)
        ends += int(((e_top[cus] == rt) & (rt > 0)).sum() + ((e_left[cus] == rl) & (rl > 0)).sum())
        assert cus.size and set(modes) <= set(range(2, 67))
    print("extensions that end at a frame edge in test 6's lists:", ends)
    assert ends >= 10
