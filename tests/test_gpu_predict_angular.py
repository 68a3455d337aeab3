"""Angular block output on the GPU (mip_predict_device_ex / mip_predict_frames_ex with
MIP_PRED_ANGULAR, mip_predicted_frames_ex): the emitted blocks are tests/angular_ref.predict's on
tests/angular_ref.boundaries bit for bit for every shape and every mode, their SAD / SATD / cost are
the engine's own angular tables, lists that mix MIP, Planar, DC, angular and rejected items write
exactly what each accepted item alone writes under every flag combination with an exact skipped
count, the 8-byte store path and unaligned rows give the same samples, the whole device chain
predicts every leaf, and the angular kernel's grid-stride loop is run beyond two rounds."""
import ctypes

import numpy as np
import pytest

import angular_ref as A
import edge_sweep_cases as E
import intra_cases as C
import intra_ref as I
import mipgpu
import predict_angular_caps as L
import predict_angular_variant_cases as V
import predict_ref as P
from mipgpu import MipEngine, layout
from predict_angular_variant_cases import (ALL_CODES, ANG_KINDS, BAD_KINDS, BASE, FILL, PER_BAD_KIND, REGULAR,  # the lists, selectors and
                                           angular_blocks, regular_blocks)                                     # expected blocks live there

pytestmark = pytest.mark.gpu

FILTER_2D = "filterFrame_2d_float_5x5_quarterCtu"


def _dev(a):
    import torch
    a = np.array(a, copy=True)                               # (the shared cases are read-only)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def _dev_items(items):
    return _dev(items.view(np.uint8))


def _host(t):
    return t.cpu().numpy().view(np.uint16)


def _sentinel(n):
    import torch
    return torch.full((n,), FILL - 65536, dtype=torch.int16, device="cuda")


def _is_angular(mode):
    mode = np.asarray(mode)
    return (mode >= BASE + 2) & (mode <= BASE + 66)


def _predict_ex(eng, d_frames, d_items, n, out, out_samples, sk, flags, refs=None):
    """mip_predict_device_ex with an explicit flags word; returns the status."""
    import torch
    s = torch.cuda.current_stream()
    return mipgpu.library().mip_predict_device_ex(eng._h, None if d_frames is None else d_frames.data_ptr(),
                                                  None if refs is None else refs.data_ptr(), 1, d_items.data_ptr(), n, out.data_ptr(),
                                                  out_samples, None if sk is None else sk.data_ptr(), flags,
                                                  ctypes.c_void_p(s.cuda_stream))


# ---------------------------------------------------------------- 1. every shape, every mode
_shape_case = V.shape_case


def test_every_shape_every_mode(gpu_available):
    """264x136, 3x2 CTUs, partial in both directions: the first row and column with the 512 and the
    replicated substitutes, the corner rule, CUs that wrap past the right edge; six CUs and more of
    every shape, all 65 modes, packed."""
    import torch
    w, h, frame, un, cus, want = _shape_case()
    shape, x, y, bw, bh = layout.cu_geometry(w, h, cus)
    assert layout.ctu_grid(w, h) == (3, 2) and w % 128 and h % 128
    assert set(shape) == set(range(layout.NUM_SHAPES))
    assert (x == 0).any() and (y == 0).any() and ((x == 0) & (y == 0)).any() and ((x > 0) & (y > 0)).any()
    assert (x + bw > w).any()                                 # wrapped CUs
    for sw, sh in ((4, 32), (32, 4), (64, 64), (4, 4)):
        assert ((bw == sw) & (bh == sh)).any(), (sw, sh)
    assert np.bincount(shape, minlength=layout.NUM_SHAPES).min() >= 6
    cu, mode = np.repeat(cus, 65), np.tile(ALL_CODES, cus.size)
    items, total = mipgpu.pred_items(w, h, 0, cu, mode)
    with MipEngine(w, h) as eng:
        out = _sentinel(total + 64)
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.predict_device(_dev(frame[None]), _dev_items(items), out[:total], skipped=sk, angular=True)
        torch.cuda.synchronize()
        got = _host(out)
        assert int(sk.item()) == 0
    assert np.all(got[total:] == FILL) and got[:total].max() <= 1023
    at = 0
    for k, c in enumerate(cus):
        blocks = got[at:at + 65 * bw[k] * bh[k]].reshape(65, bh[k], bw[k])
        bad = np.nonzero((blocks != want[int(c)]).any(axis=(1, 2)))[0]
        assert bad.size == 0, (int(c), layout.SHAPES[shape[k]].name, int(x[k]), int(y[k]), 2 + bad[:8])
        at += blocks.size
    assert at == total


# ---------------------------------------------------------------- 2. the engine's own tables
@pytest.mark.parametrize("filt,which", [(None, 0), (FILTER_2D, 0), (C.FILTER, 2)], ids=("orig", "2d_float5", "1d_int"))
def test_blocks_reproduce_the_engines_angular_tables(gpu_available, filt, which):
    """SAD, SATD and min(2 SAD, SATD) recomputed from the GPU's blocks are the entries of the
    engine's angular tables, all 65 modes: the largest shape, the most elongated ones and one of
    every size class.  With a filter the references are the engine's own.  The 2-D float 5x5 filter
    keeps these frames within 10 bits (at most 1023 on the 0 / 1023 frame), so a third case runs the
    separable integer filter on the 0 / 1023 frame, whose boundary samples reach 1535: there the
    32-bit arithmetic and the clip matter."""
    import torch
    import oracle_lib as O
    w, h = 264, 136
    frame = C.frames(w, h, 3)[which]
    if filt == C.FILTER:
        assert E.max_boundary_or_corner(O.filter_frame(frame, filt, 0), mipgpu.unavailable_cus(w, h, filt), w, h) > 1023
    lists = V.table_lists(w, h, filt)
    cu = np.concatenate([np.repeat(k, 65) for _, k in lists])
    mode = np.concatenate([np.tile(ALL_CODES, k.size) for _, k in lists])
    items, total = mipgpu.pred_items(w, h, 0, cu, mode)
    with MipEngine(w, h, filter=filt) as eng:
        host_cost = eng.angular(frame, table=True)["cost"][0]
        tab = {k: torch.empty((1, eng.cus_per_frame, 65), dtype=torch.int32, device="cuda") for k in ("cost", "sad", "satd")}
        eng.angular_device(_dev(frame[None]), **tab)
        torch.cuda.synchronize()
        tab = {k: v.cpu().numpy()[0] for k, v in tab.items()}
        got, skipped = eng.predict(frame, items, total, angular=True)
    assert skipped == 0 and got.max() <= 1023 and np.array_equal(host_cost, tab["cost"])
    pos = 0
    for s, k in lists:
        blocks = got[pos:pos + k.size * 65 * s.w * s.h].reshape(k.size, 65, s.h, s.w)
        pos += blocks.size
        _, x, y, _, _ = layout.cu_geometry(w, h, k)
        idx = (y[:, None, None] + np.arange(s.h)[None, :, None]).astype(np.int64) * w + x[:, None, None] + np.arange(s.w)[None, None, :]
        orig = frame.reshape(-1)[idx][:, None]               # [n, 1, h, w], linear indexes
        sad, satd = P.sad_blocks(orig, blocks), P.satd_blocks(orig, blocks)
        assert np.array_equal(sad, tab["sad"][k]), s.name
        assert np.array_equal(satd, tab["satd"][k]), s.name
        assert np.array_equal(np.minimum(2 * sad, satd), tab["cost"][k]), s.name
    assert pos == total


# ---------------------------------------------------------------- 3. mixed quads and the flag matrix
_mixed_case = V.mixed_case


def test_mixed_quads_and_the_flag_matrix(gpu_available):
    """One list interleaves MIP, Planar, DC, angular (both classes, both signs of the angle, the two
    PDPC modes) and rejected items, small and large blocks, so that a wave of the MIP kernel sees
    every kind in every position of its four items and a wave of the angular kernel finds its items
    scattered between entries it must leave alone.  The output tensor is twice out_samples and a
    spare frame follows the call's one."""
    import torch
    w, h, frame, un, cus, kind, cu, items, total = _mixed_case()
    n = items.size
    _, x, y, gw, gh = layout.cu_geometry(w, h, cu)
    gshape = layout.cu_geometry(w, h, cu)[0]
    is_ang = np.isin(kind, list(ANG_KINDS))
    assert items["offset"][-1] + gw[-1] * gh[-1] == total and kind[-1] == "past_end"
    out_samples = total - 1                                   # the last block is one sample too long
    for p in range(4):                                        # every kind, and both block sizes, in every quad position
        at = np.arange(p, n, 4)
        assert {"mip", "planar", "dc"} <= set(kind[at]) and set(ANG_KINDS) <= set(kind[at]) and set(BAD_KINDS) <= set(kind[at]), p
        a = at[is_ang[at]]
        assert (gw[a] * gh[a] <= 64).any() and (gw[a] * gh[a] > 64).any(), p
    quads = [set(kind[q:q + 4]) for q in range(0, n - 3, 4)]
    assert any(q & set(ANG_KINDS) and "mip" in q for q in quads) and any(q & set(ANG_KINDS) and q & {"planar", "dc"} for q in quads)
    assert any(q & set(ANG_KINDS) and q & set(BAD_KINDS) for q in quads)
    ang_want = angular_blocks(frame, w, h, cus, tuple(sorted(ANG_KINDS.values())))
    slot = {m: i for i, m in enumerate(sorted(ANG_KINDS.values()))}
    reg_want = regular_blocks(frame, w, h, cus)

    def expected(flags):
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
        return out, n - written

    d_frames, d_items = _dev(np.stack([frame, frame[::-1]])), _dev_items(items)
    lib = mipgpu.library()
    counts = {}
    with MipEngine(w, h) as eng:
        for flags in (0, 1, 4, 5):
            out = _sentinel(2 * total)
            sk = torch.zeros(1, dtype=torch.int32, device="cuda")
            assert _predict_ex(eng, d_frames, d_items, n, out, out_samples, sk, flags) == 0, lib.mip_last_error()
            torch.cuda.synchronize()
            exp, n_skipped = expected(flags)
            got = _host(out)
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, (flags, bad[:4], got[bad[:4]], exp[bad[:4]])
            assert int(sk.item()) == n_skipped, flags
            counts[flags] = n_skipped
            if flags == 0:
                old = _sentinel(2 * total)
                sk_old = torch.zeros(1, dtype=torch.int32, device="cuda")
                eng.predict_device(d_frames[:1], d_items, old[:out_samples], skipped=sk_old)   # what the old call gives today
                torch.cuda.synchronize()
                assert np.array_equal(_host(old), exp) and int(sk_old.item()) == n_skipped
        for flags in (2, 8, 6, 2 | 1, 2 | 4):                 # bit 2 never becomes a flag: errors, nothing written
            out = _sentinel(2 * total)
            sk = torch.zeros(1, dtype=torch.int32, device="cuda")
            assert _predict_ex(eng, d_frames, d_items, n, out, out_samples, sk, flags) != 0
            assert "flags" in lib.mip_last_error().decode()
            torch.cuda.synchronize()
            assert np.all(_host(out) == FILL) and int(sk.item()) == 0, flags
        # the Python flags, and a call without a skipped word
        out = _sentinel(2 * total)
        eng.predict_device(d_frames[:1], d_items, out[:out_samples], regular=True, angular=True)
        torch.cuda.synchronize()
        assert np.array_equal(_host(out), expected(5)[0])
    n_bad = len(BAD_KINDS) * PER_BAD_KIND + 1
    assert counts[5] == n_bad and counts[1] == n_bad + is_ang.sum() and counts[4] == n_bad + 2 * cus.size
    assert counts[0] == n_bad + is_ang.sum() + 2 * cus.size   # with 4 alone the Planar / DC items are skipped


# ---------------------------------------------------------------- 4. narrow stores and unaligned rows
@pytest.mark.parametrize("w,h", [(132, 136), (260, 72)], ids=("132x136", "260x72"))
def test_frame_layout_with_a_pitch_that_is_no_multiple_of_8(gpu_available, w, h):
    """W % 8 == 4: every block takes the 8-byte stores, rows start 8-byte aligned only every other
    row.  A set of CUs of mixed shapes that do not overlap, one launch, modes cycling through all 65."""
    import torch
    assert w % 8 == 4
    frame, cus, shape, x, y, bw, bh, modes, used = V.narrow_case(w, h)
    assert len(set(shape)) >= 12 and (bw >= 8).any() and (bw == 4).any() and used.mean() > 0.5
    assert set(modes) == set(range(2, 67))
    want = angular_blocks(frame, w, h, cus)
    items, n_out = mipgpu.pred_items(w, h, 0, cus, BASE + modes, layout="frame", nframes=1)
    assert n_out == w * h and np.all(items["pitch"] % 8 == 4)
    expect = np.full(w * h + 64, FILL, np.uint16)
    canvas = expect[:w * h].reshape(h, w)
    for i, c in enumerate(cus):
        canvas[y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] = want[int(c)][modes[i] - 2]
    with MipEngine(w, h) as eng:
        out = _sentinel(w * h + 64)
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.predict_device(_dev(frame[None]), _dev_items(items), out[:w * h], skipped=sk, angular=True)
        host, host_skipped = eng.predict(frame, items, n_out, angular=True)
        torch.cuda.synchronize()
        got = _host(out)
    bad = np.argwhere(got[:w * h].reshape(h, w) != canvas)
    assert bad.size == 0 and np.all(got[w * h:] == FILL), (len(bad), bad[:4])
    assert int(sk.item()) == 0 and host_skipped == 0
    assert np.array_equal(host, np.where(expect[:w * h] == FILL, mipgpu.PRED_NONE, expect[:w * h]))


def test_packed_list_of_4_wide_cus(gpu_available):
    """Packed 4-wide blocks (pitch 4): 8-byte stores of whole rows, four small blocks per wave step
    and the whole-wave path (4x32) in one list."""
    import torch
    w, h, frame, cus, bh, modes = V.four_wide_case()
    assert set(bh) == {4, 8, 16, 32}
    want = angular_blocks(frame, w, h, cus)
    items, total = mipgpu.pred_items(w, h, 0, cus, BASE + modes)
    assert np.all(items["pitch"] == 4)
    with MipEngine(w, h) as eng:
        out = _sentinel(total + 64)
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.predict_device(_dev(frame[None]), _dev_items(items), out[:total], skipped=sk, angular=True)
        torch.cuda.synchronize()
        got = _host(out)
    assert int(sk.item()) == 0 and np.all(got[total:] == FILL)
    for i, it in enumerate(items):
        blk = got[it["offset"]:it["offset"] + 4 * bh[i]].reshape(bh[i], 4)
        assert np.array_equal(blk, want[int(cus[i])][modes[i] - 2]), (int(cus[i]), int(modes[i]))


# ---------------------------------------------------------------- 5. the chain
CHAIN_KIND = "edges"                                          # the frame kind of tests/size_sweep.py for which the leaves
CHAIN_SIZES = [(264, 136)] + [tuple(s) for s in E.FIFTH]      # include angular modes of both classes and of negative angle


def _leaf_blocks(frame, w, h, mode, leaves):
    """{cu: the reference block of the leaf's kind} for the leaves `leaves` with decisions `mode`."""
    shape, x, y, _, _ = layout.cu_geometry(w, h, leaves)
    m = mode[leaves].astype(int)
    ang, reg = _is_angular(m), np.isin(m, REGULAR)
    assert np.all(m[~ang & ~reg] < 32)
    out = {}
    blocks = regular_blocks(frame, w, h, leaves[reg])
    for k, c in zip(np.nonzero(reg)[0], leaves[reg]):
        out[int(c)] = blocks[int(c)][int(m[k] == I.MODE_DC)]
    for s in layout.SHAPES:                                   # angular leaves, per shape: the modes its leaves use
        sel = np.nonzero(ang & (shape == s.index))[0]
        if sel.size:
            used = tuple(sorted(set(m[sel] - BASE)))
            blocks = angular_blocks(frame, w, h, leaves[sel], used)
            for k in sel:
                out[int(leaves[k])] = blocks[int(leaves[k])][used.index(m[k] - BASE)]
    for k in np.nonzero(~ang & ~reg)[0]:
        out[int(leaves[k])] = P.CuPredictor(frame, x[k], y[k], shape[k]).predict(m[k])
    return out


@pytest.mark.parametrize("size", CHAIN_SIZES, ids=lambda s: "%dx%d" % tuple(s))
def test_chain_predicts_every_leaf(gpu_available, size):
    """search_device -> intra_device merge -> angular_device merge (all modes, bias 0) ->
    partition_device -> predict_device(regular=True, angular=True): the partition's own list gives
    the predicted frame without a hole, and predicted_frames_ex(angular="all") gives the same
    decisions, leaves and canvas -- also on an engine whose max_batch is smaller than the call."""
    import torch
    w, h = size
    frame = E.intra_case(w, h, CHAIN_KIND)[0]
    other = E.intra_case(w, h, "noise")[0]
    with MipEngine(w, h) as eng:
        nct, ncu = eng.nctus, eng.cus_per_frame
        d_frames = _dev(frame[None])
        bm = torch.full((1, ncu), 0x5A, dtype=torch.uint8, device="cuda")
        bc = torch.full((1, ncu), -3, dtype=torch.int32, device="cuda")
        eng.search_device(d_frames, costs=False, best_mode=bm, best_cost=bc)
        eng.intra_device(d_frames, bias=E.CHAIN_BIAS, best_mode=bm, best_cost=bc)
        eng.angular_device(d_frames, bias=0, best_mode=bm, best_cost=bc)
        items = torch.zeros((1, nct, mipgpu.PART_MAX_LEAVES * mipgpu.PRED_ITEM.itemsize), dtype=torch.uint8, device="cuda")
        ctu_cost = torch.zeros((1, nct), dtype=torch.int32, device="cuda")
        ctu_leaves = torch.zeros((1, nct), dtype=torch.int32, device="cuda")
        leaf = torch.zeros((1, ncu), dtype=torch.uint8, device="cuda")
        mipgpu.partition_device(bc, w, h, penalty=E.CHAIN_PENALTY, best_mode=bm, leaf=leaf, ctu_cost=ctu_cost, ctu_leaves=ctu_leaves,
                                items=items)
        canvas = _sentinel(w * h + 64)
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.predict_device(d_frames, items, canvas[:w * h], skipped=sk, regular=True, angular=True)
        eng.check_input()
        torch.cuda.synchronize()
        one = eng.predicted_frames_ex(frame, penalty=E.CHAIN_PENALTY, bias=E.CHAIN_BIAS, angular="all")
    mode, cost = bm.cpu().numpy()[0], bc.cpu().numpy()[0]
    leaf, ctu_cost, ctu_leaves = leaf.cpu().numpy()[0].astype(bool), ctu_cost.cpu().numpy()[0], ctu_leaves.cpu().numpy()[0]
    got = _host(canvas)
    leaves = np.nonzero(leaf)[0]
    # the precondition, on the downloaded decisions: the test cannot pass empty
    ang_leaf = mode[leaves][_is_angular(mode[leaves])].astype(int) - BASE
    # (found on the CPU with tests/angular_ref.py and the C oracle: the `edges` frames give it at every one of these sizes)
    assert (ang_leaf < 34).any() and (ang_leaf >= 34).any() and any(A.ANGLE[m] < 0 for m in ang_leaf)
    assert (mode[leaves] < 32).any() and leaves.size == ctu_leaves.sum()
    assert int(sk.item()) == nct * mipgpu.PART_MAX_LEAVES - leaves.size      # the list's padding, exactly
    assert np.all(got[w * h:] == FILL)
    want = _leaf_blocks(frame, w, h, mode, leaves)
    expect = np.full((h, w), FILL, np.uint16)
    _, x, y, bw, bh = layout.cu_geometry(w, h, leaves)
    for i, c in enumerate(leaves):
        assert np.all(expect[y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] == FILL)  # leaves tile: no two share a sample
        expect[y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] = want[int(c)]
    bad = np.argwhere(got[:w * h].reshape(h, w) != expect)
    assert bad.size == 0, (len(bad), bad[:4])
    cols = layout.ctu_grid(w, h)[0]
    for ctu in np.nonzero(ctu_cost != layout.UNAVAILABLE)[0]:                # no hole inside a CTU that has a partition
        cy, cx = 128 * (ctu // cols), 128 * (ctu % cols)
        assert not np.any(expect[cy:cy + 128, cx:cx + 128] == FILL), ctu
    # the host chain: the same decisions, leaves and canvas
    assert np.array_equal(one["best_mode"][0], mode) and np.array_equal(one["best_cost"][0], cost)
    assert np.array_equal(one["leaf"][0].astype(bool), leaf) and np.array_equal(one["ctu_cost"][0], ctu_cost)
    assert np.array_equal(one["ctu_leaves"][0], ctu_leaves)
    assert np.array_equal(one["pred"][0], np.where(expect == FILL, mipgpu.PRED_NONE, expect))
    if (w, h) == (264, 136):
        frames = np.stack([frame, other, frame])
        with MipEngine(w, h, max_batch=2) as eng:            # two chunks, the second with chunk-local frame 0
            for bad_args, what in ((dict(angular=(20, 20)), "modes"), (dict(angular=(1, 2)), "modes"), (dict(angular=()), "modes"),
                                   (dict(angular="all", angular_bias=-1), "bias"),
                                   (dict(angular="all", angular_bias=(1 << 20) + 1), "bias")):
                with pytest.raises(mipgpu.MipError, match=what):
                    eng.predicted_frames_ex(frames, **bad_args)
            three = eng.predicted_frames_ex(frames, penalty=E.CHAIN_PENALTY, bias=E.CHAIN_BIAS, angular="all")
            listed = eng.predicted_frames_ex(frames[:1], penalty=E.CHAIN_PENALTY, bias=E.CHAIN_BIAS, angular=tuple(range(2, 67)))
            off = eng.predicted_frames_ex(frames[:1], penalty=E.CHAIN_PENALTY, bias=E.CHAIN_BIAS)
            plain = eng.predicted_frames(frames[:1], penalty=E.CHAIN_PENALTY, bias=E.CHAIN_BIAS)
        for key in one:
            assert np.array_equal(three[key][0], one[key][0]) and np.array_equal(three[key][2], one[key][0]), key
            assert np.array_equal(listed[key], one[key]), key
            assert np.array_equal(off[key], plain[key]), key                 # the stage off: mip_predicted_frames exactly
        assert not np.array_equal(three["pred"][1], three["pred"][0]) and _is_angular(three["best_mode"][1]).any()
        assert not _is_angular(plain["best_mode"]).any() and np.all(plain["pred"] != mipgpu.PRED_NONE)


# ---------------------------------------------------------------- 6. multi-pass
def test_multipass_scan(gpu_available):
    """A list of two rounds and a third of the angular kernel's capped grid (611 669 entries, sized
    from tests/predict_angular_caps.py), mostly partition padding: every 64-entry row holds at least
    one angular item, so every wave emits in each of its two or three passes and reuses its LDS
    words; some rows hold seven (small blocks four at a time and a remainder, large ones one by
    one) next to MIP and Planar items that the first kernel emits.  The list's last entry, in a
    partial row, is an angular item."""
    import torch
    m = V.multipass_list()
    w, h, frame, n, rows, items, total = (m[k] for k in ("w", "h", "frame", "n", "rows", "items", "total"))
    bw, bh, busy, ang_pos, per_row, at, which, kind = (m[k] for k in ("bw", "bh", "busy", "ang_pos", "per_row", "at", "which", "kind"))
    assert n == L.multipass_work(L.ENTRIES_PER_ROUND) and rows == -(-n // L.ENTRIES_PER_WAVE)
    assert n < 1 << 20 and n % L.ENTRIES_PER_WAVE and L.passes(rows, L.ROWS_PER_ROUND) == (2, 3)
    assert ang_pos.max() == n - 1 and ang_pos.size == rows + busy.size * 6
    assert per_row.min() >= 1 and per_row.max() == 7
    wave = np.arange(rows) % L.ROWS_PER_ROUND                                # every wave emits in at least two passes
    assert np.bincount(wave, weights=per_row > 0, minlength=L.ROWS_PER_ROUND).min() >= 2
    small = (bw * bh <= 64)[which]
    assert (small & (kind == 0)).any() and (~small & (kind == 0)).any() and at.size < n // 20   # a minority of the entries
    expect = V.multipass_expected(m, V.DEFAULT)
    with MipEngine(w, h) as eng:
        out = _sentinel(total + 64)
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.predict_device(_dev(frame[None]), _dev_items(items), out[:total], skipped=sk, regular=True, angular=True)
        torch.cuda.synchronize()
        got = _host(out)
        only = _sentinel(total + 64)
        sk4 = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.predict_device(_dev(frame[None]), _dev_items(items), only[:total], skipped=sk4, angular=True)
        torch.cuda.synchronize()
    bad = np.nonzero(got != expect)[0]
    assert bad.size == 0, (bad.size, bad[:4], got[bad[:4]], expect[bad[:4]])
    assert int(sk.item()) == n - at.size
    assert int(sk4.item()) == n - at.size + int((kind == 2).sum())            # flag 4 alone: the Planar items are skipped
    assert not np.any(_host(only)[:total][expect[:total] != FILL] == FILL) or (kind == 2).any()
