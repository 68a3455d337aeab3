"""Planar / DC block output on the GPU (mip_predict_device_ex / mip_predict_frames_ex with
MIP_PRED_REGULAR, mip_predicted_frames): the emitted blocks are tests/intra_ref.predict's on the
oracle's boundaries bit for bit, their SAD / SATD are the engine's own intra tables, waves that mix
MIP, regular and rejected items write exactly what each item alone writes, flags == 0 is the old
entry point, and the whole chain gives predicted frames without holes."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

import edge_sweep_cases as E
import intra_cases as C
import intra_ref as I
import mipgpu
import oracle_lib as O
import partition_ref as R
import predict_ref as P
from mipgpu import MipEngine, layout

pytestmark = pytest.mark.gpu

FILTER = C.FILTER
FILTER_2D = "filterFrame_2d_float_5x5_quarterCtu"
FILL = 0xABCD
PREFIX = np.cumsum([0] + [s.ncu for s in layout.SHAPES])
MODES = (I.MODE_PLANAR, I.MODE_DC)


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


def regular_blocks(refs, w, h, cus):
    """{cu: uint16 [2, bh, bw]} -- the Planar and the DC block of every CU of `cus` from
    intra_ref.predict on predict_ref.boundaries of refs [H, W]."""
    cus = np.asarray(cus, np.int64)
    shape, x, y, _, _ = layout.cu_geometry(w, h, cus)
    out = {}
    for s in layout.SHAPES:
        sel = np.nonzero(shape == s.index)[0]
        if not sel.size:
            continue
        b = [P.boundaries(refs, x[i], y[i], s.w, s.h)[:2] for i in sel]
        planar, dc = I.predict(np.stack([t for t, _ in b]), np.stack([l for _, l in b]), s.w, s.h)
        for j, i in enumerate(sel):
            out[int(cus[i])] = np.stack([planar[j], dc[j]]).astype(np.uint16)
    return out


def _linear(w, x, y, bw, bh):
    return ((y + np.arange(bh))[:, None] * w + x + np.arange(bw)[None, :]).reshape(-1)


# ---------------------------------------------------------------- 1. every shape, both modes, both layouts
@lru_cache(maxsize=None)
def _shape_case(w, h, filt):
    frames, refs, un, _ = C.case(w, h, filt)
    cus = P.sample_cus(w, h, un)
    return frames[1], refs[1], un, cus, regular_blocks(refs[1], w, h, cus)


@pytest.mark.parametrize("w,h,filt", [(136, 72, FILTER), (60, 36, None)], ids=("136x72-1d_int", "60x36-orig"))
def test_every_shape_both_modes_packed_and_frame_layout(gpu_available, w, h, filt):
    """Width 136: every row segment of a block of width >= 8 is 16-byte aligned in the frame layout
    (16-byte stores); width 60: the pitch is no multiple of 8 (8-byte stores)."""
    import torch
    frame, refs, un, cus, want = _shape_case(w, h, filt)
    shape, x, y, bw, bh = layout.cu_geometry(w, h, cus)
    has_available = set(layout.cu_geometry(w, h, np.nonzero(~un)[0])[0])
    assert set(shape) == has_available                        # every shape that has an available CU at this size
    if h >= 64:
        assert has_available == set(range(layout.NUM_SHAPES))  # all 47 (36 rows hold no 64x64 CU)
    else:
        assert len(has_available) >= 44 and all(layout.SHAPES[s].h <= 32 for s in has_available)
    assert ((x == 0) & (y == 0)).any() and ((x == 0) & (y > 0)).any() and ((y == 0) & (x > 0)).any()
    assert (w % 8 == 0) == (filt is not None)
    if filt is not None:
        assert refs.max() > 1023                              # the clip is exercised
    cu, mode = np.repeat(cus, 2), np.tile(MODES, cus.size)
    items, total = mipgpu.pred_items(w, h, 0, cu, mode)
    # frame layout: blocks of different shapes overlap, so the items go into layers (canvases of their
    # own launch) inside which no two blocks share a sample
    layers, used = [], []
    for i in range(cu.size):
        k = i // 2
        idx = _linear(w, x[k], y[k], bw[k], bh[k])
        for r, occ in enumerate(used):
            if not occ[idx].any():
                break
        else:
            r = len(used)
            used.append(np.zeros(w * h, bool))
            layers.append([])
        used[r][idx] = True
        layers[r].append(i)
    with MipEngine(w, h, filter=filt) as eng:
        got, skipped = eng.predict(frame, items, total, regular=True)
        out = _sentinel(total + 64)
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_frame = _dev(frame[None])
        eng.predict_device(d_frame, _dev_items(items), out[:total], skipped=sk, regular=True)
        torch.cuda.synchronize()
        assert skipped == 0 and int(sk.item()) == 0
        dev = _host(out)
        assert np.array_equal(dev[:total], got) and np.all(dev[total:] == FILL)
        for i, it in enumerate(items):
            k = i // 2
            blk = got[it["offset"]:it["offset"] + bw[k] * bh[k]].reshape(bh[k], bw[k])
            assert np.array_equal(blk, want[int(cu[i])][i % 2]), (int(cu[i]), i % 2, layout.SHAPES[shape[k]].name)
        assert got.max() <= 1023
        for r, members in enumerate(layers):
            it_r, n_r = mipgpu.pred_items(w, h, 0, cu[members], mode[members], layout="frame", nframes=1)
            assert n_r == w * h
            canvas = _sentinel(w * h + 64)
            eng.predict_device(d_frame, _dev_items(it_r), canvas[:w * h], skipped=sk, regular=True)
            host, host_skipped = eng.predict(frame, it_r, n_r, regular=True)
            expect = np.full(w * h, FILL, np.uint16)
            for i in members:
                k = i // 2
                expect[_linear(w, x[k], y[k], bw[k], bh[k])] = want[int(cu[i])][i % 2].reshape(-1)
            samples = _host(canvas)
            assert np.array_equal(samples[:w * h], expect) and np.all(samples[w * h:] == FILL), r
            assert np.array_equal(host, np.where(used[r], expect, mipgpu.PRED_NONE)) and host_skipped == 0, r
        assert int(sk.item()) == 0


# ---------------------------------------------------------------- 2. mixed list
def test_mixed_list_of_mip_regular_and_rejected_items(gpu_available):
    """MIP, Planar and DC items of small (<= 64 samples) and large shapes and eight kinds of rejected
    entries, shuffled: a wave's four items come in every mix of kinds.  The output tensor is twice
    out_samples and a spare frame follows the call's one, as in tests/test_gpu_predict.py; frame -1
    is what the partition's own padding entries carry."""
    import torch
    w, h = 136, 72
    frames, _, un, _ = C.case(w, h, None)
    frame = frames[1]
    rng = np.random.default_rng(0x3A)
    cus = P.sample_cus(w, h, un, seed=0x3A, per_shape=2)
    shape, _, _, bw, bh = layout.cu_geometry(w, h, cus)
    small = bw * bh <= 64
    assert small.any() and (~small).any()
    mip_mode = np.array([rng.integers(0, layout.SHAPES[s].total_modes) for s in shape])
    kinds = ("frame", "cu", "unavailable", "mode_ff", "mode_f2", "pitch", "offset", "past_end")
    per_kind = 10
    wide = np.nonzero(bw >= 16)[0]
    bad_cu, bad_mode, bad_kind = [], [], []
    for kind in kinds:
        for j in range(per_kind):
            pick = cus[rng.choice(wide)] if kind == "pitch" else cus[rng.integers(cus.size)]
            if kind == "unavailable":
                pick = rng.choice(np.nonzero(un)[0])
            bad_cu.append(int(pick))
            bad_mode.append(int(MODES[j % 2]) if j % 3 else 1)   # regular and MIP modes alike
            bad_kind.append(kind)
    cu = np.concatenate([cus, cus, cus, bad_cu])
    mode = np.concatenate([mip_mode, np.full(cus.size, MODES[0]), np.full(cus.size, MODES[1]), bad_mode])
    kind = np.array(["mip"] * cus.size + ["planar"] * cus.size + ["dc"] * cus.size + bad_kind)
    order = rng.permutation(cu.size)
    cu, mode, kind = cu[order], mode[order], kind[order]
    items, total = mipgpu.pred_items(w, h, 0, cu, mode)
    items["offset"][kind == "past_end"] = total - 4          # starts inside out_samples, ends past it
    items["frame"][kind == "frame"] = -1
    items["cu"][kind == "cu"] = un.size
    items["mode"][kind == "mode_ff"] = 0xFF
    items["mode"][kind == "mode_f2"] = 0xF2
    items["pitch"][kind == "pitch"] = 8
    items["offset"][kind == "offset"] += 2
    bad = np.isin(kind, kinds)
    assert bad.sum() == len(kinds) * per_kind
    quads = [tuple(sorted(set(kind[q:q + 4]))) for q in range(0, kind.size - 3, 4)]
    assert any({"mip", "planar"} <= set(q) or {"mip", "dc"} <= set(q) for q in quads)
    assert any(set(q) & set(kinds) and set(q) & {"planar", "dc"} for q in quads)
    want = regular_blocks(frame, w, h, cus)
    _, x, y, gw, gh = layout.cu_geometry(w, h, cu)
    gshape = layout.cu_geometry(w, h, cu)[0]

    def expected(regular):
        out = np.full(2 * total, FILL, np.uint16)
        n_skipped = 0
        for i, it in enumerate(items):
            k = kind[i]
            if k == "mip":
                blk = P.CuPredictor(frame, x[i], y[i], gshape[i]).predict(mode[i])
            elif k in ("planar", "dc") and regular:
                blk = want[int(cu[i])][0 if k == "planar" else 1]
            else:
                n_skipped += 1
                continue
            out[it["offset"]:it["offset"] + gw[i] * gh[i]] = blk.reshape(-1)
        return out, n_skipped

    d_frames, d_items = _dev(np.stack([frame, frame])), _dev_items(items)
    lib = mipgpu.library()
    with MipEngine(w, h) as eng:
        res = {}
        for name in ("regular", "old", "ex0"):
            out = _sentinel(2 * total)
            sk = torch.zeros(1, dtype=torch.int32, device="cuda")
            if name == "ex0":                                 # flags == 0 through the new entry point
                s = torch.cuda.current_stream()
                assert lib.mip_predict_device_ex(eng._h, d_frames.data_ptr(), None, 1, d_items.data_ptr(), items.size,
                                                 out.data_ptr(), total, sk.data_ptr(), 0, ctypes.c_void_p(s.cuda_stream)) == 0
            else:
                eng.predict_device(d_frames[:1], d_items, out[:total], skipped=sk, regular=name == "regular")
            torch.cuda.synchronize()
            res[name] = (_host(out), int(sk.item()))
        # a flag bit other than MIP_PRED_REGULAR: an error, nothing launched
        out = _sentinel(2 * total)
        s = torch.cuda.current_stream()
        assert lib.mip_predict_device_ex(eng._h, d_frames.data_ptr(), None, 1, d_items.data_ptr(), items.size, out.data_ptr(),
                                         total, None, 2 | mipgpu.PRED_REGULAR, ctypes.c_void_p(s.cuda_stream)) != 0
        assert "flags" in lib.mip_last_error().decode()
        with pytest.raises(mipgpu.MipError, match="frame"):   # the host call validates frame and cu itself
            eng.predict(frame, items, total, regular=True)
        torch.cuda.synchronize()
        assert np.all(_host(out) == FILL)
    exp, n_skipped = expected(True)
    assert n_skipped == bad.sum()
    assert res["regular"][1] == n_skipped and np.array_equal(res["regular"][0], exp)
    exp0, n_skipped0 = expected(False)
    assert n_skipped0 == bad.sum() + 2 * cus.size
    assert res["old"][1] == n_skipped0 and np.array_equal(res["old"][0], exp0)
    assert res["ex0"][1] == n_skipped0 and np.array_equal(res["ex0"][0], exp0)


# ---------------------------------------------------------------- 3. the engine's own tables
@pytest.mark.parametrize("filt", [None, FILTER_2D], ids=("orig", "2d_float5"))
def test_blocks_reproduce_the_engines_intra_tables(gpu_available, filt):
    """SAD, SATD and min(2 SAD, SATD) recomputed from the GPU's blocks are the entries of
    eng.intra(): the largest shape and the most elongated ones (the shape table has no 4x64 / 64x4;
    4x32 and 32x4 are its extremes), and one of every size class."""
    w, h = 264, 136
    frame = C.frames(w, h, 2)[0]
    nct = layout.num_ctus(w, h)
    un = mipgpu.unavailable_cus(w, h, filt).reshape(nct, layout.CUS_PER_CTU)
    names = ["ALL_AL_64x64", "ALL_AL_4x32", "ALL_AL_32x4", "ALL_AL_16x16", "ALL_NA_8x32_G2", "ALL_AL_4x4"]
    lists = []
    for n in names:
        s = layout.SHAPE_BY_NAME[n]
        ctu, c = np.nonzero(~un[:, PREFIX[s.index]:PREFIX[s.index + 1]])
        assert c.size
        lists.append((s, ctu * layout.CUS_PER_CTU + PREFIX[s.index] + c))
    cu = np.concatenate([np.repeat(k, 2) for _, k in lists])
    mode = np.concatenate([np.tile(MODES, k.size) for _, k in lists])
    items, total = mipgpu.pred_items(w, h, 0, cu, mode)
    with MipEngine(w, h, filter=filt) as eng:
        tab = eng.intra(frame, sad_satd=True)
        got, skipped = eng.predict(frame, items, total, regular=True)
    assert skipped == 0
    pos = 0
    for s, k in lists:
        blocks = got[pos:pos + k.size * 2 * s.w * s.h].reshape(k.size, 2, s.h, s.w)
        pos += blocks.size
        _, x, y, _, _ = layout.cu_geometry(w, h, k)
        idx = (y[:, None, None] + np.arange(s.h)[None, :, None]).astype(np.int64) * w + x[:, None, None] + np.arange(s.w)[None, None, :]
        orig = frame.reshape(-1)[idx][:, None]               # [n, 1, h, w], linear indexes
        sad, satd = P.sad_blocks(orig, blocks), P.satd_blocks(orig, blocks)
        assert np.array_equal(sad, tab["sad"][0][k]), s.name
        assert np.array_equal(satd, tab["satd"][0][k]), s.name
        assert np.array_equal(np.minimum(2 * sad, satd), tab["cost"][0][k]), s.name
    assert pos == total


# ---------------------------------------------------------------- 4. unaligned caller references
def _odd_view(a):
    """Device copy of `a` (uint16 frames) that starts at element 1 of a larger buffer: the device
    pointer is 2-byte but not 4-byte aligned."""
    import torch
    src = _dev(a)
    buf = torch.zeros(src.numel() + 8, dtype=src.dtype, device="cuda")
    view = buf[1:1 + src.numel()].view(src.shape)
    view.copy_(src)
    assert view.data_ptr() % 4 == 2 and view.is_contiguous()
    return view


def test_caller_references_in_a_2_byte_aligned_view(gpu_available):
    """Caller references that are not 8-byte aligned take the kernel's scalar top-row loads; the
    originals are not read (frames = None)."""
    import torch
    w, h = 136, 72
    frames, _, un, _ = C.case(w, h, None)
    refs = frames[2]                                          # another frame's samples as references
    cus = P.sample_cus(w, h, un, seed=0x44, per_shape=1)
    want = regular_blocks(refs, w, h, cus)
    shape, x, y, bw, bh = layout.cu_geometry(w, h, cus)
    mip_mode = np.array([layout.SHAPES[s].total_modes - 1 for s in shape])
    cu, mode = np.repeat(cus, 3), np.stack([np.full(cus.size, MODES[0]), mip_mode, np.full(cus.size, MODES[1])], axis=1).reshape(-1)
    items, total = mipgpu.pred_items(w, h, 0, cu, mode)
    with MipEngine(w, h) as eng:
        out = _sentinel(total)
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        view = _odd_view(refs[None])
        nbytes = items.size * mipgpu.PRED_ITEM.itemsize
        s = torch.cuda.current_stream()
        mipgpu._check(mipgpu.library().mip_predict_device_ex(eng._h, None, view.data_ptr(), 1, _dev_items(items).data_ptr(),
                                                             nbytes // mipgpu.PRED_ITEM.itemsize, out.data_ptr(), total,
                                                             sk.data_ptr(), mipgpu.PRED_REGULAR, ctypes.c_void_p(s.cuda_stream)))
        torch.cuda.synchronize()
        aligned, skipped = eng.predict(frames[0], items, total, refs=refs, regular=True)
    got = _host(out)
    assert int(sk.item()) == 0 and skipped == 0 and np.array_equal(got, aligned)
    for i, it in enumerate(items):
        k = i // 3
        blk = got[it["offset"]:it["offset"] + bw[k] * bh[k]].reshape(bh[k], bw[k])
        exp = P.CuPredictor(refs, x[k], y[k], shape[k]).predict(mode[i]) if i % 3 == 1 else want[int(cu[i])][i % 3 // 2]
        assert np.array_equal(blk, exp), (int(cu[i]), int(mode[i]))


# ---------------------------------------------------------------- 5. the chain on the device
def _filled_canvas(c, refs, w, h):
    """chain_case's canvas with the regular leaves filled from intra_ref.predict."""
    canvas = np.array(c["canvas"], copy=True)
    ks = np.nonzero(c["regular"])[0]
    blocks = regular_blocks(refs, w, h, ks)
    _, x, y, bw, bh = layout.cu_geometry(w, h, ks)
    for i, k in enumerate(ks):
        assert np.all(canvas[y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] == E.FILL)
        canvas[y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] = blocks[int(k)][0 if c["best_mode"][0, k] == I.MODE_PLANAR else 1]
    return canvas


def test_chain_on_the_device_predicts_every_leaf(gpu_available):
    """search_device -> intra_device merge -> partition_device -> predict_device(regular=True): the
    partition's own item list gives the predicted frame, regular leaves included."""
    import torch
    from test_gpu_partition import OUTPUTS, Arena
    w, h = 136, 72
    want = E.chain_case(w, h)
    leaf_modes = want["best_mode"][0][want["leaf"]]           # the precondition, on the CPU reference
    assert (leaf_modes == I.MODE_PLANAR).any() and (leaf_modes == I.MODE_DC).any() and (leaf_modes < 32).any()
    canvas_want = _filled_canvas(want, want["frame"], w, h)
    assert (want["canvas"] == E.FILL).any() and not (canvas_want == E.FILL).any()
    with MipEngine(w, h) as eng:
        nct, ncu = eng.nctus, eng.cus_per_frame
        d_frames = _dev(want["frame"][None])
        bm = torch.full((1, ncu), 0x5A, dtype=torch.uint8, device="cuda")
        bc = torch.full((1, ncu), -3, dtype=torch.int32, device="cuda")
        eng.search_device(d_frames, costs=False, best_mode=bm, best_cost=bc)
        eng.intra_device(d_frames, bias=E.CHAIN_BIAS, best_mode=bm, best_cost=bc)
        arena = Arena(1, nct)
        mipgpu.partition_device(bc, w, h, penalty=E.CHAIN_PENALTY, best_mode=bm, **{k: arena.tensor(k) for k in OUTPUTS})
        canvas = torch.full((w * h + 64,), -1, dtype=torch.int16, device="cuda")
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.predict_device(d_frames, arena.tensor("items"), canvas[:w * h], skipped=sk, regular=True)
        eng.check_input()
        got, clean = arena.read(OUTPUTS)
    assert clean
    assert np.array_equal(bm.cpu().numpy(), want["best_mode"]) and np.array_equal(bc.cpu().numpy(), want["best_cost"])
    for key in ("ctu_cost", "ctu_leaves", "items"):
        assert np.array_equal(got[key], want[key]), key
    samples = _host(canvas)
    bad = np.argwhere(samples[:w * h].reshape(h, w) != canvas_want)
    assert bad.size == 0, (len(bad), bad[:4])
    assert np.all(samples[w * h:] == E.FILL)
    assert int(sk.item()) == nct * mipgpu.PART_MAX_LEAVES - int(got["ctu_leaves"].sum())   # the padding entries only


# ---------------------------------------------------------------- 6. predicted_frames
@lru_cache(maxsize=None)
def _composition(w, h, filt):
    """The CPU composition: oracle argmin -> intra_ref.merge -> partition_ref -> predict_ref /
    intra_ref.predict, for the three frames of intra_cases."""
    frames, refs, un, tabs = C.case(w, h, filt)
    nct = layout.num_ctus(w, h)
    dec = [layout.best_modes(O.engine_search(f, filt, 0), nct) for f in frames]
    mip_mode, mip_cost = np.stack([m for m, _ in dec]), np.stack([c for _, c in dec])
    assert np.array_equal(mip_cost == layout.UNAVAILABLE, np.broadcast_to(un, mip_cost.shape))
    mode, cost = I.merge(mip_mode, mip_cost, tabs["cost"], E.CHAIN_BIAS)
    ref = R.partition_frames(cost, w, h, E.CHAIN_PENALTY, best_mode=mode)
    pred = np.full(frames.shape, mipgpu.PRED_NONE, np.uint16)
    for f in range(frames.shape[0]):
        ks = np.nonzero(ref["leaf"][f])[0]
        shape, x, y, bw, bh = layout.cu_geometry(w, h, ks)
        regular = np.isin(mode[f, ks], MODES)
        blocks = regular_blocks(refs[f], w, h, ks[regular])
        for i, k in enumerate(ks):
            if regular[i]:
                blk = blocks[int(k)][0 if mode[f, k] == I.MODE_PLANAR else 1]
            else:
                blk = P.CuPredictor(refs[f], x[i], y[i], shape[i]).predict(mode[f, k])
            assert np.all(pred[f, y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] == mipgpu.PRED_NONE)
            pred[f, y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] = blk
    out = dict(best_mode=mode, best_cost=cost, leaf=ref["leaf"], ctu_cost=ref["ctu_cost"], ctu_leaves=ref["ctu_leaves"], pred=pred)
    return frames, out


CHAIN_CASES = [(136, 72, None), (60, 36, None), (136, 72, FILTER), (60, 36, FILTER), (136, 64, FILTER), (72, 64, FILTER)]


@pytest.mark.parametrize("w,h,filt", CHAIN_CASES, ids=lambda v: "orig" if v is None else str(v)[-6:])
def test_predicted_frames_equal_the_cpu_composition(gpu_available, w, h, filt):
    """3 different frames on max_batch = 2: two chunks, the second with chunk-local frame index 0
    for the call's frame 2.  With the separable filter at a height that is no multiple of 32 the CUs
    that read the last frame rows are unavailable and no CTU of these sizes can be tiled: every
    sample stays MIP_PRED_NONE.  The two sizes of height 64 give the filtered chain leaves: at 136x64
    one CTU has a partition and the other has none, at 72x64 every sample is predicted."""
    frames, want = _composition(w, h, filt)
    assert not np.array_equal(frames[0], frames[2])
    leaf_modes = want["best_mode"][want["leaf"].astype(bool)]
    has = want["ctu_cost"] != layout.UNAVAILABLE
    if filt is None or h % 32 == 0:
        assert np.isin(leaf_modes, MODES).any() and (leaf_modes < 32).any() and has.any(axis=1).all()
        assert not np.array_equal(want["pred"][0], want["pred"][2])
        assert has.all() == ((w, h) != (136, 64))
    else:
        assert not has.any() and np.all(want["pred"] == mipgpu.PRED_NONE)
    with MipEngine(w, h, filter=filt, max_batch=2) as eng:
        for penalty, bias, what in ((-1, None, "penalty"), ((1 << 20) + 1, None, "penalty"), (None, (0, -1), "bias"),
                                    (None, ((1 << 20) + 1, 0), "bias")):
            with pytest.raises(mipgpu.MipError, match=what):
                eng.predicted_frames(frames, penalty=penalty, bias=bias)
        got = eng.predicted_frames(frames, penalty=E.CHAIN_PENALTY, bias=E.CHAIN_BIAS)
        last = eng.predicted_frames(frames[2:], penalty=E.CHAIN_PENALTY, bias=E.CHAIN_BIAS)
    assert sorted(got) == sorted(want)
    for key in want:
        assert np.array_equal(got[key], want[key]), key
        assert np.array_equal(last[key], want[key][2:]), key
    covered = np.zeros(frames.shape, bool)
    f, k = np.nonzero(want["leaf"])
    _, x, y, bw, bh = layout.cu_geometry(w, h, k)
    for i in range(k.size):
        covered[f[i], y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] = True
    # (filtered boundary samples above 1023 enter the MIP upsampling, so only the sentinel is excluded)
    assert np.all(got["pred"][~covered] == mipgpu.PRED_NONE) and np.all(got["pred"][covered] != mipgpu.PRED_NONE)
