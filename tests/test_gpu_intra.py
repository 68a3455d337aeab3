"""Planar / DC baseline costs and the decision merge on the GPU (mip_intra_device /
mip_intra_frames): the whole tables equal the numpy restatement (tests/intra_ref.py, pinned by
tests/test_intra_cpu.py) bit for bit, device and host calls agree, nothing but the outputs
asked for is written, the merge follows the numpy rule, and the merged decisions run through
partition and prediction unchanged."""
import numpy as np
import pytest

import intra_cases as C
import intra_ref as I
import mipgpu
import partition_ref as R
from mipgpu import MipEngine, layout

pytestmark = pytest.mark.gpu

FILTER = C.FILTER
GUARD = 64                      # int32 words before and after every output (keeps 8-byte alignment)
GUARD_WORD = -0x5A5A5A5B
UN = layout.UNAVAILABLE


def _dev(a):
    import torch
    a = np.array(a, copy=True)                               # (the shared cases are read-only)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


class Arena:
    """The three tables inside one guard-filled int32 device buffer, so that a write outside a
    table -- or into a table that was not passed -- shows."""

    def __init__(self, nframes, ncu):
        import torch
        self.n, self.shape = nframes * ncu * 2, (nframes, ncu, 2)
        self.at = {k: GUARD + i * (self.n + GUARD) for i, k in enumerate(C.TABLES)}
        self.buf = torch.full((GUARD + 3 * (self.n + GUARD),), GUARD_WORD, dtype=torch.int32, device="cuda")

    def tensor(self, key):
        return self.buf[self.at[key]:self.at[key] + self.n]

    def read(self, given):
        """(tables of `given` as numpy, True if every word outside them is still the guard)."""
        import torch
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        clean = np.ones(host.size, bool)
        out = {}
        for key in given:
            clean[self.at[key]:self.at[key] + self.n] = False
            out[key] = host[self.at[key]:self.at[key] + self.n].reshape(self.shape)
        return out, bool(np.all(host[clean] == GUARD_WORD))


def _tables(eng, frames, refs=None, given=C.TABLES):
    arena = Arena(frames.shape[0], eng.cus_per_frame)
    eng.intra_device(_dev(frames), refs=None if refs is None else _dev(refs), **{k: arena.tensor(k) for k in given})
    return arena.read(given)


def _max_boundary(refs, un, w, h):
    """Largest boundary sample of every available CU of refs [H, W] (0 for the others)."""
    flat = refs.reshape(-1).astype(np.int64)
    _, x, y, bw, bh = layout.cu_geometry(w, h, np.arange(un.size))
    out = np.zeros(un.size, np.int64)
    for k in np.nonzero(~un)[0]:
        top = flat[(y[k] - 1) * w + x[k]:(y[k] - 1) * w + x[k] + bw[k]] if y[k] > 0 else flat[x[k] - 1:x[k]] if x[k] > 0 else flat[:0]
        left = flat[y[k] * w + x[k] - 1:(y[k] + bh[k]) * w + x[k] - 1:w] if x[k] > 0 else flat[(y[k] - 1) * w:(y[k] - 1) * w + 1] if y[k] > 0 else flat[:0]
        out[k] = max(top.max(initial=512), left.max(initial=512))
    return out


@pytest.mark.parametrize("filt", (None, FILTER), ids=("orig", "1d_int"))
def test_full_tables_device_and_host(gpu_available, filt):
    """136x72: two CTU columns, partial CTUs right and below, wrapped CUs.  All 3 x 2 x 5380 x 2
    entries of every table, device and host call."""
    w, h = 136, 72
    frames, refs, un, ref = C.case(w, h, filt)
    _, x, y, _, _ = layout.cu_geometry(w, h, np.arange(un.size))
    ok = ~un
    assert (ok & (x == 0) & (y == 0)).any() and (ok & (x == 0) & (y > 0)).any() and (ok & (y == 0) & (x > 0)).any()
    assert (ok & (x + 4 > w)).any()                           # CUs right of the frame (wrapped samples)
    if filt is not None:                                      # the clip is exercised
        assert max(_max_boundary(r, un, w, h).max() for r in refs) > 1023
    with MipEngine(w, h, filter=filt, max_batch=3) as eng:
        got, clean = _tables(eng, frames)
        host = eng.intra(frames, sad_satd=True)
        only_cost = eng.intra(frames[1:])
    assert clean
    for key in C.TABLES:
        assert np.array_equal(got[key], ref[key]), key
        assert np.array_equal(host[key], ref[key]), key
        assert np.array_equal(got[key][:, :, 0] == UN, np.broadcast_to(un, got[key].shape[:2])), key
    assert list(only_cost) == ["cost"] and np.array_equal(only_cost["cost"], ref["cost"][1:])
    assert np.array_equal(ref["cost"], np.where(ref["sad"] == UN, UN, np.minimum(2 * ref["sad"].astype(np.int64), ref["satd"])))


def test_caller_references_and_chunked_host_call(gpu_available):
    """Caller references equal to the oracle-filtered frames give the engine-filter result on
    every CU available in both sets; the host call of 3 frames on max_batch = 2 runs two chunks."""
    w, h = 136, 72
    frames, refs, un_f, ref_f = C.case(w, h, FILTER)
    un_o = mipgpu.unavailable_cus(w, h)
    both = ~un_f & ~un_o
    assert both.any() and (un_f & ~un_o).any()
    with MipEngine(w, h, max_batch=2) as eng:
        got, clean = _tables(eng, frames[:2], refs=refs[:2])
        host = eng.intra(frames, refs=refs, sad_satd=True)
    assert clean
    for key in C.TABLES:
        assert np.array_equal(got[key][:, both], ref_f[key][:2][:, both]), key
        assert np.array_equal(host[key][:, both], ref_f[key][:, both]), key
        assert np.array_equal(host[key][:2], got[key]), key
        assert np.array_equal(host[key][:, :, 1] == UN, np.broadcast_to(un_o, host[key].shape[:2])), key


@pytest.mark.parametrize("given", [("sad",), ("cost", "satd"), ("satd",)], ids="+".join)
def test_tables_not_asked_for_are_not_written(gpu_available, given):
    w, h = 136, 72
    frames, _, _, ref = C.case(w, h, None)
    with MipEngine(w, h, max_batch=3) as eng:
        got, clean = _tables(eng, frames, given=given)
    assert clean
    for key in given:
        assert np.array_equal(got[key], ref[key]), key


def _decisions(eng, d_frames):
    import torch
    n = d_frames.shape[0]
    bm = torch.full((n, eng.cus_per_frame), 0x5A, dtype=torch.uint8, device="cuda")
    bc = torch.full((n, eng.cus_per_frame), -3, dtype=torch.int32, device="cuda")
    eng.search_device(d_frames, costs=False, best_mode=bm, best_cost=bc)
    return bm, bc


def test_merge_follows_the_rule(gpu_available):
    import torch
    w, h = 136, 72
    frames, _, un, ref = C.case(w, h, None)
    with MipEngine(w, h, max_batch=3) as eng:
        d_frames = _dev(frames)
        bm, bc = _decisions(eng, d_frames)
        bm0, bc0 = bm.cpu().numpy(), bc.cpu().numpy()
        assert np.array_equal(bc0 == UN, np.broadcast_to(un, bc0.shape)) and np.all(bm0[bc0 == UN] == 0xFF)
        for bias in (None, (0, 0), (1 << 20, 0), (40, 25)):
            m, c = bm.clone(), bc.clone()
            assert eng.intra_device(d_frames, bias=bias, best_mode=m, best_cost=c) is None   # merge only
            wm, wc = I.merge(bm0, bc0, ref["cost"], bias)
            assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(c.cpu().numpy(), wc), bias
            assert np.array_equal(wm[:, un], bm0[:, un])
            if bias in (None, (0, 0)):
                assert (wm == I.MODE_PLANAR).any() and (wm == I.MODE_DC).any() and (wm < 32).any()
            if bias == (1 << 20, 0):
                assert not (wm == I.MODE_PLANAR).any() and (wm == I.MODE_DC).any()
        # tables and merge in one call
        arena = Arena(3, eng.cus_per_frame)
        m, c = bm.clone(), bc.clone()
        eng.intra_device(d_frames, cost=arena.tensor("cost"), best_mode=m, best_cost=c)
        got, clean = arena.read(("cost",))
        wm, wc = I.merge(bm0, bc0, ref["cost"])
        assert clean and np.array_equal(got["cost"], ref["cost"])
        assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(c.cpu().numpy(), wc)
        # a bias outside 0 .. 1<<20 is refused before any launch
        for bad in ((-1, 0), (0, (1 << 20) + 1)):
            m, c = bm.clone(), bc.clone()
            with pytest.raises(mipgpu.MipError, match="bias"):
                eng.intra_device(d_frames, bias=bad, best_mode=m, best_cost=c)
            torch.cuda.synchronize()
            assert torch.equal(m, bm) and torch.equal(c, bc)
        with pytest.raises(mipgpu.MipError, match="together"):
            eng.intra_device(d_frames, best_cost=bc.clone())


def test_merge_ties_on_a_uniform_frame(gpu_available):
    """Uniform frame: Planar and DC cost the same on every CU (0 away from the frame's first row
    and column), the MIP decision costs 0 or a small constant b per shape.  Zero-cost MIP
    decisions tie and stay (strictly lower only); with bias (b, b) the CUs at MIP cost b tie and
    stay, costlier ones become Planar (DC ties Planar and comes later); with (b, b - 1) both
    kinds become DC."""
    w, h, v = 136, 72, 700
    frame = np.full((1, h, w), v, np.uint16)
    un = mipgpu.unavailable_cus(w, h)
    ref = I.tables(frame[0], frame[0], un)["cost"][None]
    _, x, y, _, _ = layout.cu_geometry(w, h, np.arange(un.size))
    flat = ~un & (x > 0) & (y > 0)
    assert np.array_equal(ref[..., 0], ref[..., 1]) and not ref[0, flat].any()
    with MipEngine(w, h) as eng:
        d_frames = _dev(frame)
        bm, bc = _decisions(eng, d_frames)
        bm0, bc0 = bm.cpu().numpy(), bc.cpu().numpy()
        values, counts = np.unique(bc0[0, flat], return_counts=True)
        assert values[0] == 0 and values.size > 2              # ties at 0, and costs above and below b
        b = int(values[1:][np.argmax(counts[1:])])
        assert 0 < b < values[-1]
        for bias in ((0, 0), (b, b), (b, b - 1)):
            m, c = bm.clone(), bc.clone()
            eng.intra_device(d_frames, bias=bias, best_mode=m, best_cost=c)
            wm, wc = I.merge(bm0, bc0, ref, bias)
            assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(c.cpu().numpy(), wc), bias
            at_b, above = flat & (bc0[0] == b), flat & (bc0[0] > b)
            zero = flat & (bc0[0] == 0)
            assert np.array_equal(wm[0, zero], bm0[0, zero]) and np.array_equal(wm[0, un], bm0[0, un])
            if bias == (0, 0):
                assert np.all(wm[0, at_b] == I.MODE_PLANAR) and np.all(wc[0, at_b] == 0)
            elif bias == (b, b):
                assert np.all(wm[0, above] == I.MODE_PLANAR) and np.all(wc[0, above] == b)
                assert np.array_equal(wm[0, at_b], bm0[0, at_b]) and np.all(wc[0, at_b] == b)
            else:
                assert np.all(wm[0, above | at_b] == I.MODE_DC) and np.all(wc[0, above | at_b] == b - 1)
        # constant MIP costs of 5: (3, 3) Planar, (3, 2) DC, (5, 5) ties MIP, (5, 4) DC
        five = np.where(un, UN, 5).astype(np.int32)[None]
        mode5 = np.where(un, 0xFF, 1).astype(np.uint8)[None]
        for bias, want in (((3, 3), I.MODE_PLANAR), ((3, 2), I.MODE_DC), ((5, 5), 1), ((5, 4), I.MODE_DC)):
            m, c = _dev(mode5), _dev(five)
            eng.intra_device(d_frames, bias=bias, best_mode=m, best_cost=c)
            wm, wc = I.merge(mode5, five, ref, bias)
            assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(c.cpu().numpy(), wc), bias
            assert np.all(wm[0, flat] == want) and np.all(wm[0, un] == 0xFF), bias


def test_merged_decisions_feed_partition_and_prediction(gpu_available):
    import torch
    w, h, penalty = 136, 72, 600
    frames = C.frames(w, h)[:1]
    with MipEngine(w, h) as eng:
        d_frames = _dev(frames)
        bm, bc = _decisions(eng, d_frames)
        eng.intra_device(d_frames, bias=(30, 30), best_mode=bm, best_cost=bc)
        nct = eng.nctus
        items = torch.zeros((1, nct, mipgpu.PART_MAX_LEAVES * mipgpu.PRED_ITEM.itemsize), dtype=torch.uint8, device="cuda")
        ctu_cost = torch.zeros((1, nct), dtype=torch.int32, device="cuda")
        ctu_leaves = torch.zeros((1, nct), dtype=torch.int32, device="cuda")
        leaf = torch.zeros((1, eng.cus_per_frame), dtype=torch.uint8, device="cuda")
        mipgpu.partition_device(bc, w, h, penalty=penalty, best_mode=bm, leaf=leaf, ctu_cost=ctu_cost, ctu_leaves=ctu_leaves,
                                items=items)
        canvas = torch.full((w * h,), -1, dtype=torch.int16, device="cuda")
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.predict_device(d_frames, items, canvas, skipped=sk)
        eng.check_input()
        torch.cuda.synchronize()
    mode, cost, leaf = bm.cpu().numpy(), bc.cpu().numpy(), leaf.cpu().numpy().astype(bool)
    ref = R.partition_frames(cost, w, h, penalty)
    assert np.array_equal(ctu_cost.cpu().numpy(), ref["ctu_cost"]) and np.array_equal(leaf, ref["leaf"].astype(bool))
    regular = leaf & ((mode == I.MODE_PLANAR) | (mode == I.MODE_DC))
    assert regular.any() and (leaf & ~regular).any()          # leaves of both kinds
    padding = nct * mipgpu.PART_MAX_LEAVES - int(ctu_leaves.sum().item())
    assert int(sk.item()) == padding + int(regular.sum())
    # the regular-mode leaves' samples stay unwritten, the MIP leaves' are predicted
    got = canvas.cpu().numpy().view(np.uint16).reshape(h, w)
    _, x, y, bw, bh = layout.cu_geometry(w, h, np.nonzero(leaf[0])[0])
    for k, cu in enumerate(np.nonzero(leaf[0])[0]):
        blk = got[y[k]:y[k] + bh[k], x[k]:x[k] + bw[k]]
        assert np.all(blk == 0xFFFF) if regular[0, cu] else np.all(blk <= 1023), int(cu)


def test_second_geometry_two_frames(gpu_available):
    """264x136, two frames in one call: frame indexing and a CTU grid of more than one row."""
    w, h = 264, 136
    frames, _, un, ref = C.case(w, h, None, 2)
    assert layout.ctu_grid(w, h) == (3, 2)
    with MipEngine(w, h, max_batch=2) as eng:
        got, clean = _tables(eng, frames)
    assert clean
    for key in C.TABLES:
        assert np.array_equal(got[key], ref[key]), key
    assert not np.array_equal(got["cost"][0], got["cost"][1])


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


def test_unaligned_frames_and_references(gpu_available):
    """The kernel stages frames and references with 2-byte loads, so it asks no alignment of
    the caller's frames (mip_intra.hip header): frames, and frames plus caller references, at an
    odd sample offset give the tables of the aligned call."""
    w, h = 136, 72
    frames, _, un, ref = C.case(w, h, None)
    caller = frames[::-1]                                     # another frame's samples as references
    want = [I.tables(f, r, un) for f, r in zip(frames[:2], caller[:2])]
    with MipEngine(w, h, max_batch=3) as eng:
        arena = Arena(3, eng.cus_per_frame)
        eng.intra_device(_odd_view(frames), **{k: arena.tensor(k) for k in C.TABLES})
        got, clean = arena.read(C.TABLES)
        arena_r = Arena(2, eng.cus_per_frame)
        eng.intra_device(_odd_view(frames[:2]), refs=_odd_view(caller[:2]), **{k: arena_r.tensor(k) for k in C.TABLES})
        got_r, clean_r = arena_r.read(C.TABLES)
    assert clean and clean_r
    for key in C.TABLES:
        assert np.array_equal(got[key], ref[key]), key
        assert np.array_equal(got_r[key], np.stack([t[key] for t in want])), key
    assert not np.array_equal(got_r["cost"], got["cost"][:2])


def test_intra_and_search_share_the_filter_scratch_on_two_streams(gpu_available):
    """intra_device on one stream and search_device on another, both filtering into the engine's
    reference scratch (no caller references), different frames, alternating: each launch waits
    for the previous reader of the scratch (refs_done), so each gives its own reference."""
    import torch
    import oracle_lib as O
    from mipgpu.synth import synth_frames
    w, h = 136, 72
    frames, _, un, ref = C.case(w, h, FILTER)
    other = synth_frames(w, h, 2, 0x2B7, 0)
    want = np.stack([O.engine_search(f, FILTER, 0) for f in other])
    assert not np.array_equal(other[0], frames[0])
    rounds = 6
    with MipEngine(w, h, filter=FILTER, max_batch=3) as eng:
        d_intra = [_dev(np.roll(frames, -i, axis=0)) for i in range(3)]
        d_search = [_dev(other[::s]) for s in (1, -1)]
        arenas = [Arena(3, eng.cus_per_frame) for _ in range(rounds)]
        costs = [torch.full((2, eng.costs_per_frame), -7, dtype=torch.int32, device="cuda") for _ in range(rounds)]
        torch.cuda.synchronize()                              # inputs and prefills ran on the current stream
        s_intra, s_search = torch.cuda.Stream(), torch.cuda.Stream()
        for i in range(rounds):
            eng.intra_device(d_intra[i % 3], stream=s_intra, **{k: arenas[i].tensor(k) for k in C.TABLES})
            eng.search_device(d_search[i % 2], costs=costs[i], stream=s_search)
        torch.cuda.synchronize()
        eng.check_input(stream=s_search)
        for i in range(rounds):
            got, clean = arenas[i].read(C.TABLES)
            assert clean, i
            for key in C.TABLES:
                assert np.array_equal(got[key], np.roll(ref[key], -(i % 3), axis=0)), (i, key)
            assert np.array_equal(costs[i].cpu().numpy(), want[::1 if i % 2 == 0 else -1]), i


def test_bad_arguments_fail_before_any_launch(gpu_available):
    """More frames than max_batch on an engine that filters, a table pointer that is 4-byte but
    not 8-byte aligned, and no output at all: an error each, nothing written."""
    import ctypes
    import torch
    w, h = 136, 72
    frames = C.frames(w, h)
    with MipEngine(w, h, filter=FILTER, max_batch=2) as eng:
        n = eng.cus_per_frame
        d_frames = _dev(frames)
        arena = Arena(3, n)
        bm = torch.full((3, n), 0x5A, dtype=torch.uint8, device="cuda")
        bc = torch.full((3, n), -3, dtype=torch.int32, device="cuda")
        with pytest.raises(mipgpu.MipError, match="max_batch"):
            eng.intra_device(d_frames, best_mode=bm, best_cost=bc, **{k: arena.tensor(k) for k in C.TABLES})
        for key in C.TABLES:                                  # one table 4 bytes off, the others as they should be
            outs = {k: arena.tensor(k)[:2 * n * 2] for k in C.TABLES}
            outs[key] = arena.buf[arena.at[key] + 1:arena.at[key] + 1 + 2 * n * 2]
            assert outs[key].data_ptr() % 8 == 4
            with pytest.raises(mipgpu.MipError, match="8-byte aligned"):
                eng.intra_device(d_frames[:2], best_mode=bm[:2], best_cost=bc[:2], **outs)
        # no output: the Python call would allocate `cost`, so this one goes to the C entry point
        s = torch.cuda.current_stream()
        rc = mipgpu.library().mip_intra_device(eng._h, d_frames.data_ptr(), None, 2, None, None, None, None, None, None,
                                               ctypes.c_void_p(s.cuda_stream))
        assert rc != 0 and "no output" in mipgpu.library().mip_last_error().decode()
        _, clean = arena.read(())
        assert clean
        assert torch.all(bm == 0x5A) and torch.all(bc == -3)
        # the engine still works
        got = eng.intra_device(d_frames[:2])
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), C.case(w, h, FILTER)[3]["cost"][:2])
