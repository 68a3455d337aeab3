"""VVC's 4-tap angular interpolation on the GPU (mip_angular_interp, MIP_ANG_INTERP_4TAP): the cost
kernel, the refined search, the block output and the two host chains, bit for bit against the numpy
restatement tests/angular_tap4_ref.py (pinned by tests/test_angular_tap4_cpu.py, which also shows on
the restatements alone that these cases are not vacuous), under both reference settings; every
frame-edge residue of tests/size_sweep.py; a multi-pass batch; and the switch in stream order."""
import numpy as np
import pytest

import angular_cases as AC
import angular_ref as A
import angular_refine_ref as RR
import angular_tap4_cases as TC
import angular_tap4_ref as T
import candidates_ref as K
import edge_sweep_cases as E
import launch_caps as L
import mipgpu
import predict_ref as P
import size_sweep as S
from mipgpu import MipEngine, layout

pytestmark = pytest.mark.gpu

W, H = TC.SIZE
BASE = mipgpu.MODE_ANGULAR_BASE
PAIR = ("ang_mode", "ang_cost")
ALL_OUT = TC.TABLES + PAIR
TAP4, TAP2 = mipgpu.ANG_INTERP_4TAP, mipgpu.ANG_INTERP_2TAP
BOTH = pytest.mark.parametrize("refs_setting", (TC.EXT, TC.SUB), ids=("extended", "substituted"))


def _dev(a):
    import torch
    a = np.array(a, copy=True)                               # (the shared cases are read-only)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def _outputs(n, ncu, tried=False):
    import torch
    out = {k: torch.full((n, ncu, 65), -7, dtype=torch.int32, device="cuda") for k in TC.TABLES}
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


def _engine(w, h, refs_setting, **kw):
    eng = MipEngine(w, h, **kw)
    eng.angular_refs = refs_setting
    eng.angular_interp = TAP4
    return eng


# ---------------------------------------------------------------- 1. the cost kernel
@BOTH
def test_cost_kernel_tables_pair_and_merge(gpu_available, refs_setting):
    """264x136, 3 frames, all 65 modes: the three tables and the ang pair; the merge after a search;
    the odd-length list; a refused value; and with the switch off again the outputs are those of an
    engine that never touched it, GPU against GPU."""
    frames, _, un, _, _, ref = TC.case(W, H, refs_setting)
    with MipEngine(W, H, max_batch=3) as eng, MipEngine(W, H, max_batch=3) as plain:
        eng.angular_refs = plain.angular_refs = refs_setting
        assert eng.angular_interp == TAP2
        before = _costs(eng, frames)
        eng.angular_interp = TAP4
        assert eng.angular_interp == TAP4 and plain.angular_interp == TAP2 and eng.angular_refs == refs_setting
        got = _costs(eng, frames)
        host = eng.angular(frames, table=True)
        odd = _costs(eng, frames, modes=TC.ODD_LENGTH_LIST)
        d_frames = _dev(frames)
        bm, bc = _decisions(eng, d_frames)
        bm0, bc0 = bm.cpu().numpy(), bc.cpu().numpy()
        eng.angular_device(d_frames, bias=30, best_mode=bm, best_cost=bc)
        merged = bm.cpu().numpy(), bc.cpu().numpy()
        for bad in (2, -1):
            with pytest.raises(mipgpu.MipError, match="unknown angular interpolation setting"):
                eng.angular_interp = bad
        assert eng.angular_interp == TAP4
        eng.angular_interp = TAP2
        back = _costs(eng, frames)
        never = _costs(plain, frames)
    _same(got, ref)
    _same(host, ref, ("cost",) + PAIR)
    _same(odd, TC.listed(ref, TC.ODD_LENGTH_LIST))
    want = A.merge(bm0, bc0, ref["ang_mode"], ref["ang_cost"], 30)
    assert np.array_equal(merged[0], want[0]) and np.array_equal(merged[1], want[1])
    assert ((merged[0] >= 0x82) & (merged[0] <= 0xC2)).any() and (merged[0][:, ~un] < 32).any()
    _same(back, never)
    _same(before, never)
    assert not np.array_equal(got["cost"], never["cost"])
    for slot in (16, 48):                                                                       # modes 18 and 50
        assert np.array_equal(got["cost"][:, :, slot], never["cost"][:, :, slot])
    _, _, bw, bh = layout.cu_geometry(W, H, np.arange(un.size))[1:]
    small = (bw * bh <= 32)                                                                     # 4x4, 4x8, 8x4: size class 2
    for slot in (0, 32, 64):                                                                    # modes 2, 34 and 66
        assert np.array_equal(got["cost"][:, small, slot], never["cost"][:, small, slot])
        assert not np.array_equal(got["cost"][:, ~small, slot], never["cost"][:, ~small, slot])


@BOTH
@pytest.mark.parametrize("source", (TC.XC.FILTER_2D, "caller"), ids=("2d_int", "caller_refs"))
def test_cost_kernel_with_an_engine_filter_and_with_caller_references(gpu_available, source, refs_setting):
    frames, refs, _, _, _, ref = TC.case(W, H, refs_setting, source, 2, TC.ODD_LENGTH_LIST)
    with _engine(W, H, refs_setting, filter=TC.XC.FILTER_2D, max_batch=2) as eng:
        got = _costs(eng, frames, refs=refs if source == "caller" else None, modes=TC.ODD_LENGTH_LIST)
        host = eng.angular(frames, refs=refs if source == "caller" else None, modes=TC.ODD_LENGTH_LIST, table=True)
    _same(got, ref)
    _same(host, ref, ("cost",) + PAIR)


# ---------------------------------------------------------------- 2. the refine kernel
@BOTH
def test_refine_kernel(gpu_available, refs_setting):
    """The even list, seeds 1 and 3: tables, pair, tried and the merge, against the refinement rule of
    tests/angular_refine_ref.py over the 4-tap 65-mode tables."""
    frames, _, un, _, _, full = TC.case(W, H, refs_setting)
    with _engine(W, H, refs_setting, max_batch=3) as eng:
        d_frames = _dev(frames)
        bm, bc = _decisions(eng, d_frames)
        bm0, bc0 = bm.cpu().numpy(), bc.cpu().numpy()
        for seeds in (1, 3):
            want = RR.refine(full, TC.EVEN_MODES, seeds)
            got = _costs(eng, frames, modes=TC.EVEN_MODES, seeds=seeds)
            _same(got, want, ALL_OUT + ("tried",), seeds)
            m, c = bm.clone(), bc.clone()
            eng.angular_refine_device(d_frames, modes=TC.EVEN_MODES, seeds=seeds, bias=12, best_mode=m, best_cost=c)
            wm, wc = A.merge(bm0, bc0, want["ang_mode"], want["ang_cost"], 12)
            assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(c.cpu().numpy(), wc), seeds
        host = eng.angular_refine(frames, modes=TC.EVEN_MODES, seeds=3, table=True)
    _same(host, want, ("cost", "tried") + PAIR)
    assert (want["tried"][:, ~un] > 33).all() and ((want["ang_mode"] != 0xFF) & (want["ang_mode"] % 2 == 1)).any()   # a candidate (odd mode) wins


# ---------------------------------------------------------------- 3. block output
def _block_cus(un, e_top, e_left, per=2):
    """CUs of every shape over the combinations of full / partial / zero lengths that exist."""
    picked = TC.XC.length_class_cus(W, H, un, e_top, e_left, per)
    assert set(layout.cu_geometry(W, H, picked)[0]) == set(range(layout.NUM_SHAPES))
    return picked


def _blocks(refs, cus, e_top, e_left, modes):
    """{cu: uint16 [len(modes), bh, bw]} of the restatement."""
    shape, x, y, _, _ = layout.cu_geometry(W, H, cus)
    out = {}
    for s in layout.SHAPES:
        sel = np.nonzero(shape == s.index)[0]
        if sel.size:
            top, left, corner = T.X.boundaries(refs, x[sel], y[sel], s.w, s.h, e_top[cus[sel]], e_left[cus[sel]])
            blocks = T.predict(top, left, corner, s.w, s.h, modes).astype(np.uint16)
            for j, i in enumerate(sel):
                out[int(cus[i])] = blocks[:, j]
    return out


@BOTH
def test_block_output_packed_and_frame_layout(gpu_available, refs_setting):
    """264x136, 2 frames.  Packed: CUs of every shape, the modes of BLOCK_MODES, plus items of
    unavailable CUs that are skipped and counted; the blocks are the restatement's and their SAD /
    SATD against the originals the table entries.  Frame layout: the 16x16 CUs tile the canvas."""
    frames, _, un, e_top, e_left, ref = TC.case(W, H, refs_setting)
    frames = frames[:2]
    cus = _block_cus(un, *TC.inputs(W, H)[3:])
    modes = np.array(TC.BLOCK_MODES)
    dead = np.nonzero(un)[0][::997][:20]
    cu = np.concatenate([np.repeat(cus, modes.size), dead])
    mode = np.concatenate([np.tile(BASE + modes, cus.size), np.full(dead.size, BASE + 66)])
    _, x, y, bw, bh = layout.cu_geometry(W, H, cus)
    s16 = layout.SHAPE_BY_NAME["ALL_AL_16x16"]
    shape_all, xa, ya, _, _ = layout.cu_geometry(W, H, np.arange(un.size))
    tile = np.nonzero(~un & (shape_all == s16.index) & (xa + 16 <= W))[0]
    tile_mode = modes[np.arange(tile.size) % modes.size]
    with _engine(W, H, refs_setting, max_batch=2) as eng:
        got = {}
        for f in (0, 1):
            items, total = mipgpu.pred_items(W, H, 0, cu, mode)
            got[f] = eng.predict(frames[f], items, total, angular=True)
        items, total = mipgpu.pred_items(W, H, 1, tile, BASE + tile_mode, layout="frame", nframes=2)
        canvas, skipped = eng.predict(frames, items, total, angular=True)
    for f in (0, 1):
        out, skipped_f = got[f]
        assert skipped_f == dead.size
        want = _blocks(frames[f], cus, e_top, e_left, TC.BLOCK_MODES)
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
    for m in TC.BLOCK_MODES:
        k = tile[tile_mode == m]
        for c, b in _blocks(frames[1], k, e_top, e_left, (m,)).items():
            expect[ya[c]:ya[c] + 16, xa[c]:xa[c] + 16] = b[0]
    assert np.array_equal(canvas[1], expect)


# ---------------------------------------------------------------- 4. the chains
@BOTH
def test_chains_equal_the_composition_of_the_device_calls(gpu_available, refs_setting):
    """predicted_frames_ex(angular="all") and candidates(k=3, angular=EVEN, seeds=1) follow the switch
    with no setting of their own: they equal the device calls composed by hand on the same engine,
    and the restatement -- the angular merge is the 4-tap pair's, every angular leaf's block the 4-tap
    predictor's, the candidate lists those of tests/candidates_ref.py over the 4-tap refined table --
    and differ from the same chain with the switch off."""
    import torch
    frames, _, un, e_top, e_left, full = TC.case(W, H, refs_setting)
    frames = frames[:2]
    bias, penalty, ang_bias = E.CHAIN_BIAS, E.CHAIN_PENALTY, 0
    with _engine(W, H, refs_setting, max_batch=2) as eng:
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
        cand = eng.candidates(frames, k=3, angular=TC.EVEN_MODES, seeds=1)
        intra = torch.empty((2, ncu, 2), dtype=torch.int32, device="cuda")
        eng.intra_device(d_frames, cost=intra)
        eng.angular_interp = TAP2
        chain_off = eng.predicted_frames_ex(frames, penalty=penalty, bias=bias, angular="all", angular_bias=ang_bias)
        cand_off = eng.candidates(frames, k=3, angular=TC.EVEN_MODES, seeds=1)
        intra = intra.cpu().numpy()
    mode, cost, leaf = bm.cpu().numpy(), bc.cpu().numpy(), leaf.cpu().numpy()
    wm, wc = A.merge(pm, pc, full["ang_mode"][:2], full["ang_cost"][:2], ang_bias)
    assert np.array_equal(mode, wm) and np.array_equal(cost, wc)
    assert np.array_equal(chain["best_mode"], mode) and np.array_equal(chain["best_cost"], cost)
    assert np.array_equal(chain["leaf"], leaf)
    pred = canvas.cpu().numpy().view(np.uint16).reshape(2, H, W)
    assert np.array_equal(chain["pred"], pred)
    assert not np.array_equal(chain_off["best_cost"], chain["best_cost"]) and not np.array_equal(chain_off["pred"], chain["pred"])
    assert not np.array_equal(cand_off["costs"], cand["costs"])
    fractional_leaves = 0
    for f in (0, 1):
        leaves = np.nonzero(leaf[f].astype(bool) & (mode[f] >= BASE + 2) & (mode[f] <= BASE + 66))[0]
        for m in np.unique(mode[f][leaves]):
            k = leaves[mode[f][leaves] == m]
            _, kx, ky, kw, kh = layout.cu_geometry(W, H, k)
            for c, b in _blocks(frames[f], k, e_top, e_left, (int(m) - BASE,)).items():
                j = int(np.nonzero(k == c)[0][0])
                assert np.array_equal(pred[f, ky[j]:ky[j] + kh[j], kx[j]:kx[j] + kw[j]], b[0]), (f, int(c), int(m))
            fractional_leaves += k.size * (int(m) - BASE in T.FRACTIONAL_MODES)
    assert fractional_leaves > 20
    with MipEngine(W, H, max_batch=2) as eng:
        alone = eng.candidates(frames, k=3, regular=False)
    fine = RR.refine({k: v[:2] for k, v in full.items()}, TC.EVEN_MODES, 1)["cost"]
    want = K.candidates(3, alone["modes"], alone["costs"], intra, None, fine, 0)
    assert np.array_equal(cand["modes"], want[0]) and np.array_equal(cand["costs"], want[1])
    assert ((cand["modes"] >= BASE + 2) & (cand["modes"] <= BASE + 66) & (cand["modes"] % 2 == 1)).any()   # refined (odd) modes are listed


# ---------------------------------------------------------------- 5. frame edges
def _sweep(w, h, refs_setting, refine):
    frame, un, _, _, ref = TC.sweep_case(w, h, refs_setting, None if refine else TC.SWEEP_LIST)
    with _engine(w, h, refs_setting) as eng:
        got = _costs(eng, frame[None], modes=TC.SWEEP_LIST)
        fine = _costs(eng, frame[None], modes=TC.SWEEP_LIST, seeds=2) if refine else None
    _same({k: v[0] for k, v in got.items()}, TC.listed(ref, TC.SWEEP_LIST) if refine else ref, note=(w, h, refs_setting))
    if refine:
        want = RR.refine({k: v[None] for k, v in ref.items()}, TC.SWEEP_LIST, 2)
        _same(fine, want, ALL_OUT + ("tried",), (w, h, refs_setting))


@pytest.mark.parametrize("size", S.ALL_SIZES, ids=S.size_id)
def test_every_frame_edge_residue_with_extended_lines(gpu_available, size):
    """The 70 sizes, one noise frame, both classes and both signs of the angle through the cost
    kernel; every fifth size also through the refined search (seeds 2; the candidates leave the list)."""
    _sweep(size[0], size[1], TC.EXT, size in S.ALL_SIZES[::5])


@pytest.mark.parametrize("size", S.ALL_SIZES[::5], ids=S.size_id)
def test_frame_edge_residues_with_substituted_lines(gpu_available, size):
    _sweep(size[0], size[1], TC.SUB, True)


# ---------------------------------------------------------------- 6. multi-pass
@BOTH
def test_multipass(gpu_available, refs_setting):
    """2 1/3 rounds of the launcher's capped grid at 136x136 with a two-mode list: every workgroup
    runs two or three passes over its reused LDS window, going between 64x64 and 32x32 items, with
    the coefficient words staged once.  The frames repeat with period 2; compared on the device."""
    import torch
    w, h, modes = 136, 136, (3, 65)
    frames, _, un, _, _, full = TC.case(w, h, refs_setting, None, 2)
    ref = TC.listed(full, modes)
    unit = layout.num_ctus(w, h) * AC.ANGULAR_ITEMS_PER_CTU
    cap = AC.angular_cap(torch.cuda.get_device_properties(0).multi_processor_count)
    nframes = -(-L.multipass_work(cap) // unit)
    assert L.passes(nframes * unit, cap)[0] >= 2
    sel = np.arange(nframes) % 2
    with _engine(w, h, refs_setting, max_batch=nframes) as eng:
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
    modes = TC.ODD_LENGTH_LIST
    frames, _, _, _, _, ref = TC.case(W, H, TC.EXT, None, 2, modes)
    two = TC.XC.case(W, H, None, 2, modes)[5]
    assert not np.array_equal(ref["cost"], two["cost"])
    with MipEngine(W, H, max_batch=2) as eng:
        eng.angular_refs = TC.EXT
        d_frames = _dev(frames)
        first, second, third = (_outputs(2, eng.cus_per_frame) for _ in range(3))
        torch.cuda.synchronize()
        eng.angular_interp = TAP4
        eng.angular_device(d_frames, modes=modes, **first)
        eng.angular_interp = TAP2
        eng.angular_device(d_frames, modes=modes, **second)
        eng.angular_interp = TAP4
        eng.angular_device(d_frames, modes=modes, **third)
        got = [_host(o) for o in (first, second, third)]
    _same(got[0], ref)
    _same(got[1], two)
    _same(got[2], ref)
