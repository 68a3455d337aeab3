"""Extended angular reference lines on the GPU (mip_angular_refs, MIP_ANG_REFS_EXTENDED): the cost
kernel, the refined search, the block output and the two host chains, bit for bit against the numpy
restatement tests/angular_ext_ref.py (pinned by tests/test_angular_ext_cpu.py, which also shows on
the restatements alone that these cases are not vacuous); every frame-edge residue of
tests/size_sweep.py; a multi-pass batch; and the switch in stream order."""
import numpy as np
import pytest

import angular_cases as AC
import angular_ext_cases as XC
import angular_ext_ref as X
import angular_ref as A
import angular_refine_ref as RR
import candidates_ref as K
import edge_sweep_cases as E
import launch_caps as L
import mipgpu
import predict_ref as P
import size_sweep as S
from mipgpu import MipEngine, layout

pytestmark = pytest.mark.gpu

W, H = XC.SIZE
BASE = mipgpu.MODE_ANGULAR_BASE
PAIR = ("ang_mode", "ang_cost")
ALL_OUT = XC.TABLES + PAIR
EXT, SUB = mipgpu.ANG_REFS_EXTENDED, mipgpu.ANG_REFS_SUBSTITUTED


def _dev(a):
    import torch
    a = np.array(a, copy=True)                               # (the shared cases are read-only)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def _outputs(n, ncu, tried=False):
    import torch
    out = {k: torch.full((n, ncu, 65), -7, dtype=torch.int32, device="cuda") for k in XC.TABLES}
    out["ang_mode"] = torch.full((n, ncu), 0x5A, dtype=torch.uint8, device="cuda")
    out["ang_cost"] = torch.full((n, ncu), -7, dtype=torch.int32, device="cuda")
    if tried:
        out["tried"] = torch.full((n, ncu), 0x5A, dtype=torch.uint8, device="cuda")
    return out


def _host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _costs(eng, frames, refs=None, modes=None, seeds=None):
    """Every output of angular_device (seeds None) or angular_refine_device as numpy."""
    out = _outputs(frames.shape[0], eng.cus_per_frame, tried=seeds is not None)
    d_refs = None if refs is None else _dev(refs)
    if seeds is None:
        eng.angular_device(_dev(frames), modes=modes, refs=d_refs, **out)
    else:
        eng.angular_refine_device(_dev(frames), modes=modes, seeds=seeds, refs=d_refs, **out)
    return _host(out)


def _decisions(eng, d_frames):
    import torch
    n = d_frames.shape[0]
    bm = torch.full((n, eng.cus_per_frame), 0x5A, dtype=torch.uint8, device="cuda")
    bc = torch.full((n, eng.cus_per_frame), -3, dtype=torch.int32, device="cuda")
    eng.search_device(d_frames, costs=False, best_mode=bm, best_cost=bc)
    return bm, bc


def _same(got, want, keys=ALL_OUT, note=None):
    for key in keys:
        assert np.array_equal(got[key], want[key]), (key, note)


# ---------------------------------------------------------------- 1. the cost kernel
def test_cost_kernel_tables_pair_and_merge(gpu_available):
    """264x136, 3 frames, all 65 modes: the three tables and the ang pair; the merge after a search;
    an odd-length list; the switch set back gives the substituted path's outputs, GPU against GPU
    (an engine that never saw the switch)."""
    frames, _, un, e_top, e_left, ref = XC.case(W, H)
    with MipEngine(W, H, max_batch=3) as eng, MipEngine(W, H, max_batch=3) as plain:
        assert eng.angular_refs == SUB
        before = _costs(eng, frames)
        eng.angular_refs = EXT
        assert eng.angular_refs == EXT and plain.angular_refs == SUB
        got = _costs(eng, frames)
        host = eng.angular(frames, table=True)
        odd = _costs(eng, frames, modes=XC.ODD_LENGTH_LIST)
        d_frames = _dev(frames)
        bm, bc = _decisions(eng, d_frames)
        bm0, bc0 = bm.cpu().numpy(), bc.cpu().numpy()
        eng.angular_device(d_frames, bias=30, best_mode=bm, best_cost=bc)
        merged = bm.cpu().numpy(), bc.cpu().numpy()
        with pytest.raises(mipgpu.MipError, match="unknown angular reference setting"):
            eng.angular_refs = 2
        assert eng.angular_refs == EXT
        eng.angular_refs = SUB
        back = _costs(eng, frames)
        never = _costs(plain, frames)
    _same(got, ref)
    _same(host, ref, ("cost",) + PAIR)
    _same(odd, XC.listed(ref, XC.ODD_LENGTH_LIST))
    want = A.merge(bm0, bc0, ref["ang_mode"], ref["ang_cost"], 30)
    assert np.array_equal(merged[0], want[0]) and np.array_equal(merged[1], want[1])
    assert ((merged[0] >= 0x82) & (merged[0] <= 0xC2)).any() and (merged[0][:, ~un] < 32).any()
    _same(back, never)
    _same(before, never)
    assert not np.array_equal(got["cost"], never["cost"])
    assert np.array_equal(got["cost"][:, :, 16:49], never["cost"][:, :, 16:49])                 # modes 18..50
    assert np.array_equal(got["cost"][:, (e_top == 0) & (e_left == 0)], never["cost"][:, (e_top == 0) & (e_left == 0)])


@pytest.mark.parametrize("source", (XC.FILTER_2D, "caller"), ids=("2d_int", "caller_refs"))
def test_cost_kernel_with_an_engine_filter_and_with_caller_references(gpu_available, source):
    """The engine filter's lengths go with its availability and undefined-sample sets; caller
    references with the MIP_FILTER_NONE sets, on an engine that has a filter of its own."""
    frames, refs, _, _, _, ref = XC.case(W, H, source, 2, XC.ODD_LENGTH_LIST)
    with MipEngine(W, H, filter=XC.FILTER_2D, max_batch=2) as eng:
        eng.angular_refs = EXT
        got = _costs(eng, frames, refs=refs if source == "caller" else None, modes=XC.ODD_LENGTH_LIST)
        host = eng.angular(frames, refs=refs if source == "caller" else None, modes=XC.ODD_LENGTH_LIST, table=True)
    _same(got, ref)
    _same(host, ref, ("cost",) + PAIR)


# ---------------------------------------------------------------- 2. the refine kernel
def test_refine_kernel(gpu_available):
    """The even list, seeds 1..3: tables, pair, tried and the merge, against the refinement rule of
    tests/angular_refine_ref.py over the extended 65-mode tables."""
    frames, _, un, _, _, full = XC.case(W, H)
    with MipEngine(W, H, max_batch=3) as eng:
        eng.angular_refs = EXT
        d_frames = _dev(frames)
        bm, bc = _decisions(eng, d_frames)
        bm0, bc0 = bm.cpu().numpy(), bc.cpu().numpy()
        for seeds in (1, 2, 3):
            want = RR.refine(full, XC.EVEN_MODES, seeds)
            got = _costs(eng, frames, modes=XC.EVEN_MODES, seeds=seeds)
            _same(got, want, ALL_OUT + ("tried",), seeds)
            m, c = bm.clone(), bc.clone()
            eng.angular_refine_device(d_frames, modes=XC.EVEN_MODES, seeds=seeds, bias=12, best_mode=m, best_cost=c)
            wm, wc = A.merge(bm0, bc0, want["ang_mode"], want["ang_cost"], 12)
            assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(c.cpu().numpy(), wc), seeds
        host = eng.angular_refine(frames, modes=XC.EVEN_MODES, seeds=3, table=True)
    _same(host, want, ("cost", "tried") + PAIR)
    assert (want["tried"][:, ~un] > 33).all() and ((want["ang_mode"] != 0xFF) & (want["ang_mode"] % 2 == 1)).any()   # a candidate (odd mode) wins


# ---------------------------------------------------------------- 3. block output
def _block_cus(un, e_top, e_left, per=2):
    """CUs of every shape over the nine combinations of full / partial / zero lengths, where they exist."""
    picked = XC.length_class_cus(W, H, un, e_top, e_left, per)
    shape, _, _, bw, bh = layout.cu_geometry(W, H, picked)
    assert set(XC.length_class(e_top[picked], bh)) == {0, 1, 2} == set(XC.length_class(e_left[picked], bw))
    assert set(shape) == set(range(layout.NUM_SHAPES))
    return picked


def _blocks(refs, cus, e_top, e_left, modes):
    """{cu: uint16 [len(modes), bh, bw]} of the restatement."""
    shape, x, y, _, _ = layout.cu_geometry(W, H, cus)
    out = {}
    for s in layout.SHAPES:
        sel = np.nonzero(shape == s.index)[0]
        if sel.size:
            top, left, corner = X.boundaries(refs, x[sel], y[sel], s.w, s.h, e_top[cus[sel]], e_left[cus[sel]])
            blocks = X.predict(top, left, corner, s.w, s.h, modes).astype(np.uint16)
            for j, i in enumerate(sel):
                out[int(cus[i])] = blocks[:, j]
    return out


def test_block_output_packed_and_frame_layout(gpu_available):
    """264x136, 2 frames.  Packed: CUs of every shape with full, partial and zero lengths on both
    lines, the modes 2, 10, 17, 18, 34, 50, 51, 58, 66, plus items of unavailable CUs that are
    skipped and counted; the blocks are the restatement's and their SAD / SATD the table entries.
    Frame layout: the 16x16 CUs tile the canvas, one mode each."""
    frames, _, un, e_top, e_left, ref = XC.case(W, H)
    frames = frames[:2]
    cus = _block_cus(un, e_top, e_left)
    modes = np.array(XC.BLOCK_MODES)
    dead = np.nonzero(un)[0][::997][:20]
    cu = np.concatenate([np.repeat(cus, modes.size), dead])
    mode = np.concatenate([np.tile(BASE + modes, cus.size), np.full(dead.size, BASE + 66)])
    _, x, y, bw, bh = layout.cu_geometry(W, H, cus)
    s16 = layout.SHAPE_BY_NAME["ALL_AL_16x16"]
    shape_all, xa, ya, _, _ = layout.cu_geometry(W, H, np.arange(un.size))
    tile = np.nonzero(~un & (shape_all == s16.index) & (xa + 16 <= W))[0]
    tile_mode = modes[np.arange(tile.size) % modes.size]
    with MipEngine(W, H, max_batch=2) as eng:
        eng.angular_refs = EXT
        got = {}
        for f in (0, 1):
            items, total = mipgpu.pred_items(W, H, 0, cu, mode)
            got[f] = eng.predict(frames[f], items, total, angular=True)
        items, total = mipgpu.pred_items(W, H, 1, tile, BASE + tile_mode, layout="frame", nframes=2)
        canvas, skipped = eng.predict(frames, items, total, angular=True)
    for f in (0, 1):
        out, skipped_f = got[f]
        assert skipped_f == dead.size
        want = _blocks(frames[f], cus, e_top, e_left, XC.BLOCK_MODES)
        at = 0
        for i, c in enumerate(cus):
            blocks = out[at:at + modes.size * bw[i] * bh[i]].reshape(modes.size, bh[i], bw[i])
            at += blocks.size
            assert np.array_equal(blocks, want[int(c)]), (f, int(c), int(x[i]), int(y[i]), int(e_top[c]), int(e_left[c]))
            idx = (y[i] + np.arange(bh[i])[:, None]).astype(np.int64) * W + x[i] + np.arange(bw[i])[None, :]
            orig = frames[f].reshape(-1)[idx][None]
            assert np.array_equal(P.sad_blocks(orig, blocks), ref["sad"][f, c, modes - 2]), (f, int(c))
            assert np.array_equal(P.satd_blocks(orig, blocks), ref["satd"][f, c, modes - 2]), (f, int(c))
        assert np.all(out[at:] == mipgpu.PRED_NONE)                                          # the skipped items' blocks
    assert skipped == 0 and total == 2 * W * H
    canvas = canvas.reshape(2, H, W)
    assert np.all(canvas[0] == mipgpu.PRED_NONE)
    expect = np.full((H, W), mipgpu.PRED_NONE, np.uint16)
    for m in XC.BLOCK_MODES:
        k = tile[tile_mode == m]
        for c, b in _blocks(frames[1], k, e_top, e_left, (m,)).items():
            expect[ya[c]:ya[c] + 16, xa[c]:xa[c] + 16] = b[0]
    assert np.array_equal(canvas[1], expect) and (e_top[tile] > 0).any() and (e_left[tile] > 0).any()


# ---------------------------------------------------------------- 4. the chains
def test_chains_equal_the_composition_of_the_device_calls(gpu_available):
    """predicted_frames_ex(angular="all") and candidates(k=3, angular=EVEN, seeds=1) with the switch
    on: the device calls composed by hand on the same engine, and the restatement -- the angular
    merge is the extended pair's, every angular leaf's block the extended predictor's, and the
    candidate lists those of tests/candidates_ref.py over the extended refined table."""
    import torch
    frames, _, un, e_top, e_left, full = XC.case(W, H)
    frames = frames[:2]
    bias, penalty, ang_bias = E.CHAIN_BIAS, E.CHAIN_PENALTY, 0
    with MipEngine(W, H, max_batch=2) as eng:
        eng.angular_refs = EXT
        nct, ncu = eng.nctus, eng.cus_per_frame
        d_frames = _dev(frames)
        bm, bc = _decisions(eng, d_frames)
        eng.intra_device(d_frames, bias=bias, best_mode=bm, best_cost=bc)
        pm, pc = bm.cpu().numpy(), bc.cpu().numpy()
        eng.angular_device(d_frames, bias=ang_bias, best_mode=bm, best_cost=bc)
        items = torch.zeros((2, nct, mipgpu.PART_MAX_LEAVES * mipgpu.PRED_ITEM.itemsize), dtype=torch.uint8, device="cuda")
        leaf = torch.zeros((2, ncu), dtype=torch.uint8, device="cuda")
        mipgpu.partition_device(bc, W, H, penalty=penalty, best_mode=bm, leaf=leaf, items=items)
        canvas = torch.full((2 * W * H,), -1, dtype=torch.int16, device="cuda")              # MIP_PRED_NONE
        eng.predict_device(d_frames, items, canvas, regular=True, angular=True)
        torch.cuda.synchronize()
        chain = eng.predicted_frames_ex(frames, penalty=penalty, bias=bias, angular="all", angular_bias=ang_bias)
        # candidates: the MIP lists of the search's table, the Planar / DC table, the refined angular table
        cand = eng.candidates(frames, k=3, angular=XC.EVEN_MODES, seeds=1)
        intra = torch.empty((2, ncu, 2), dtype=torch.int32, device="cuda")
        eng.intra_device(d_frames, cost=intra)
        eng.angular_refs = SUB
        chain_sub = eng.predicted_frames_ex(frames, penalty=penalty, bias=bias, angular="all", angular_bias=ang_bias)
        intra = intra.cpu().numpy()
    mode, cost, leaf = bm.cpu().numpy(), bc.cpu().numpy(), leaf.cpu().numpy()
    # the restatement: the merge of the extended pair into the decisions after the Planar / DC merge
    wm, wc = A.merge(pm, pc, full["ang_mode"][:2], full["ang_cost"][:2], ang_bias)
    assert np.array_equal(mode, wm) and np.array_equal(cost, wc)
    assert np.array_equal(chain["best_mode"], mode) and np.array_equal(chain["best_cost"], cost)
    assert np.array_equal(chain["leaf"], leaf)
    pred = canvas.cpu().numpy().view(np.uint16).reshape(2, H, W)
    assert np.array_equal(chain["pred"], pred)
    assert not np.array_equal(chain_sub["best_cost"], chain["best_cost"]) and not np.array_equal(chain_sub["pred"], chain["pred"])
    # every angular leaf's block is the extended predictor's; some have a real extension
    extended_leaves = 0
    for f in (0, 1):
        leaves = np.nonzero(leaf[f].astype(bool) & (mode[f] >= BASE + 2) & (mode[f] <= BASE + 66))[0]
        for m in np.unique(mode[f][leaves]):
            k = leaves[mode[f][leaves] == m]
            _, kx, ky, kw, kh = layout.cu_geometry(W, H, k)
            for c, b in _blocks(frames[f], k, e_top, e_left, (int(m) - BASE,)).items():
                j = int(np.nonzero(k == c)[0][0])
                assert np.array_equal(pred[f, ky[j]:ky[j] + kh[j], kx[j]:kx[j] + kw[j]], b[0]), (f, int(c), int(m))
                positive = A.ANGLE[int(m) - BASE] > 0
                extended_leaves += bool(positive and (e_top[c] if m - BASE >= 34 else e_left[c]))
    assert extended_leaves > 20
    # the candidate lists: the search's MIP decision lists of length 3 come from the engine itself
    # (flags == 0 gives them alone); the other two families from the restatements
    with MipEngine(W, H, max_batch=2) as eng:
        alone = eng.candidates(frames, k=3, regular=False)
    fine = RR.refine({k: v[:2] for k, v in full.items()}, XC.EVEN_MODES, 1)["cost"]
    want = K.candidates(3, alone["modes"], alone["costs"], intra, None, fine, 0)
    assert np.array_equal(cand["modes"], want[0]) and np.array_equal(cand["costs"], want[1])
    assert ((cand["modes"] >= BASE + 2) & (cand["modes"] <= BASE + 66) & (cand["modes"] % 2 == 1)).any()   # refined (odd) modes are listed


# ---------------------------------------------------------------- 5. frame edges
def _sweep_engine_outputs(w, h, filt, which):
    frame, refs, un, e_top, e_left, ref = XC.sweep_case(w, h, filt)
    out = {}
    with MipEngine(w, h, filter=filt) as eng:
        eng.angular_refs = EXT
        out["cost"] = _costs(eng, frame[None], modes=XC.SWEEP_LIST)
        if which == "all":
            out["refine"] = _costs(eng, frame[None], modes=XC.SWEEP_LIST, seeds=2)
            cus = np.nonzero(~un)[0][::37]
            modes = np.array(XC.SWEEP_LIST)[np.arange(cus.size) % len(XC.SWEEP_LIST)]
            items, total = mipgpu.pred_items(w, h, 0, cus, BASE + modes)
            out["blocks"] = (cus, modes) + eng.predict(frame, items, total, angular=True)
    return frame, refs, un, e_top, e_left, ref, out


@pytest.mark.parametrize("size", S.ALL_SIZES, ids=S.size_id)
def test_every_frame_edge_residue(gpu_available, size):
    """The 70 sizes, one frame, both classes' positive angles plus 18 / 34 / 50, through the cost
    kernel; every fifth size also through the refine and the block-output kernels."""
    w, h = size
    fifth = size in S.ALL_SIZES[::5]
    frame, refs, un, e_top, e_left, ref, out = _sweep_engine_outputs(w, h, None, "all" if fifth else "cost")
    _same({k: v[0] for k, v in out["cost"].items()}, ref)
    if not fifth:
        return
    full = X.tables(frame, refs, un, e_top, e_left)                 # (the candidates leave the list)
    full["ang_mode"], full["ang_cost"] = A.best(full["cost"])
    want = RR.refine({k: v[None] for k, v in full.items()}, XC.SWEEP_LIST, 2)
    _same(out["refine"], want, ALL_OUT + ("tried",))
    cus, modes, got, skipped = out["blocks"]
    assert skipped == 0
    _, x, y, bw, bh = layout.cu_geometry(w, h, cus)
    at = 0
    for i, c in enumerate(cus):
        block = got[at:at + bw[i] * bh[i]].reshape(bh[i], bw[i])
        at += block.size
        assert np.array_equal(block, X.predict_cu(refs, x[i], y[i], bw[i], bh[i], e_top[c], e_left[c], int(modes[i]))), (int(c), int(modes[i]))


@pytest.mark.parametrize("size", S.ALL_SIZES[::5], ids=S.size_id)
@pytest.mark.parametrize("filt", (E.FILTER_SEP, E.FILTER_2D), ids=("1d_int", "2d_float5"))
def test_frame_edge_residues_with_an_engine_filter(gpu_available, size, filt):
    w, h = size
    _, _, _, _, _, ref, out = _sweep_engine_outputs(w, h, filt, "cost")
    _same({k: v[0] for k, v in out["cost"].items()}, ref)


# ---------------------------------------------------------------- 6. multi-pass
def test_multipass(gpu_available):
    """2 1/3 rounds of the launcher's capped grid at 136x136 with a two-mode list: every workgroup
    runs two or three passes over its reused LDS window and its extension cells, going between 64x64
    and 32x32 items.  The frames repeat with period 2; compared on the device."""
    import torch
    w, h, modes = 136, 136, (2, 66)
    frames, _, un, e_top, e_left, full = XC.case(w, h, None, 2)
    ref = XC.listed(full, modes)
    unit = layout.num_ctus(w, h) * AC.ANGULAR_ITEMS_PER_CTU
    cap = AC.angular_cap(torch.cuda.get_device_properties(0).multi_processor_count)
    nframes = -(-L.multipass_work(cap) // unit)
    assert L.passes(nframes * unit, cap)[0] >= 2 and (e_top[~un] > 0).any() and (e_left[~un] > 0).any()
    sel = np.arange(nframes) % 2
    with MipEngine(w, h, max_batch=nframes) as eng:
        eng.angular_refs = EXT
        ncu = eng.cus_per_frame
        cost = torch.full((nframes, ncu, 65), -7, dtype=torch.int32, device="cuda")
        am = torch.full((nframes, ncu), 0x5A, dtype=torch.uint8, device="cuda")
        ac = torch.full((nframes, ncu), -7, dtype=torch.int32, device="cuda")
        eng.angular_device(_dev(frames[sel]), modes=modes, cost=cost, ang_mode=am, ang_cost=ac)
        want = _dev(ref["cost"])
        for f0 in range(0, nframes, 32):
            same = cost[f0:f0 + 32] == want[torch.from_numpy(sel[f0:f0 + 32]).cuda()]
            assert bool(same.all()), (f0, torch.nonzero(~same)[:4].cpu().numpy())
        tried = torch.full((nframes, ncu), 0x5A, dtype=torch.uint8, device="cuda")
        fine_mode, fine_cost = am.clone(), ac.clone()
        eng.angular_refine_device(_dev(frames[sel]), modes=modes, seeds=1, ang_mode=fine_mode, ang_cost=fine_cost, tried=tried)
        got_am, got_ac = am.cpu().numpy(), ac.cpu().numpy()
        got_fm, got_fc, got_tried = fine_mode.cpu().numpy(), fine_cost.cpu().numpy(), tried.cpu().numpy()
    assert np.array_equal(got_am, ref["ang_mode"][sel]) and np.array_equal(got_ac, ref["ang_cost"][sel])
    want = RR.refine(full, modes, 1)
    assert np.array_equal(got_fm, want["ang_mode"][sel]) and np.array_equal(got_fc, want["ang_cost"][sel])
    assert np.array_equal(got_tried, want["tried"][sel])


# ---------------------------------------------------------------- 7. the setting in stream order
def test_each_call_keeps_the_setting_it_was_enqueued_with(gpu_available):
    """A call with the switch on, the switch flipped, a second call on the same stream, nothing
    waited for in between: each output is its own setting's."""
    import torch
    modes = XC.ODD_LENGTH_LIST
    frames, _, _, _, _, ref = XC.case(W, H, None, 2, modes)
    sub = XC.substituted(W, H, None, 2, modes)
    assert not np.array_equal(ref["cost"], sub["cost"])
    with MipEngine(W, H, max_batch=2) as eng:
        d_frames = _dev(frames)
        first, second, third = (_outputs(2, eng.cus_per_frame) for _ in range(3))
        torch.cuda.synchronize()
        eng.angular_refs = EXT
        eng.angular_device(d_frames, modes=modes, **first)
        eng.angular_refs = SUB
        eng.angular_device(d_frames, modes=modes, **second)
        eng.angular_refs = EXT
        eng.angular_device(d_frames, modes=modes, **third)
        got = [_host(o) for o in (first, second, third)]
    _same(got[0], ref)
    _same(got[1], sub)
    _same(got[2], ref)
