"""Angular intra costs, the best angular mode and its merge on the GPU (mip_angular_device /
mip_angular_frames): whole tables equal the numpy restatement (tests/angular_ref.py, pinned by
tests/test_angular_cpu.py) bit for bit, device and host calls agree, nothing but the outputs
asked for is written, mode lists leave the other slots unavailable, the merge follows the numpy
rule -- after a search and after a Planar / DC merge -- and the merged decisions run through
partition and prediction unchanged."""
import ctypes

import numpy as np
import pytest

import angular_cases as AC
import angular_ref as A
import mipgpu
import partition_ref as R
from mipgpu import MipEngine, layout

pytestmark = pytest.mark.gpu

FILTER = AC.FILTER
GUARD = 64                      # elements before and after every output
GUARD_WORD, GUARD_BYTE = -0x5A5A5A5B, 0x5A
UN = layout.UNAVAILABLE
INT32_OUT = AC.TABLES + ("ang_cost",)
ALL_OUT = INT32_OUT + ("ang_mode",)


def _dev(a):
    import torch
    a = np.array(a, copy=True)                               # (the shared cases are read-only)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


class Arena:
    """The three tables and ang_cost inside one guard-filled int32 device buffer, ang_mode inside
    a guard-filled uint8 one, so that a write outside an output -- or into one that was not
    passed -- shows."""

    def __init__(self, nframes, ncu):
        import torch
        self.size = {k: nframes * ncu * (1 if k.startswith("ang") else 65) for k in ALL_OUT}
        self.shape = {k: (nframes, ncu) if k.startswith("ang") else (nframes, ncu, 65) for k in ALL_OUT}
        self.at, end = {}, GUARD
        for k in INT32_OUT:
            self.at[k], end = end, end + self.size[k] + GUARD
        self.at["ang_mode"] = GUARD
        self.buf = torch.full((end,), GUARD_WORD, dtype=torch.int32, device="cuda")
        self.bytes = torch.full((self.size["ang_mode"] + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")

    def tensor(self, key):
        src = self.bytes if key == "ang_mode" else self.buf
        return src[self.at[key]:self.at[key] + self.size[key]]

    def outputs(self, given):
        return {k: self.tensor(k) for k in given}

    def read(self, given):
        """(outputs of `given` as numpy, True if every element outside them is still the guard)."""
        import torch
        torch.cuda.synchronize()
        words, octets = self.buf.cpu().numpy(), self.bytes.cpu().numpy()
        clean_w, clean_b = np.ones(words.size, bool), np.ones(octets.size, bool)
        out = {}
        for key in given:
            host, clean = (octets, clean_b) if key == "ang_mode" else (words, clean_w)
            clean[self.at[key]:self.at[key] + self.size[key]] = False
            out[key] = host[self.at[key]:self.at[key] + self.size[key]].reshape(self.shape[key])
        return out, bool(np.all(words[clean_w] == GUARD_WORD) and np.all(octets[clean_b] == GUARD_BYTE))


def _run(eng, frames, refs=None, modes=None, given=ALL_OUT):
    arena = Arena(frames.shape[0], eng.cus_per_frame)
    eng.angular_device(_dev(frames), refs=None if refs is None else _dev(refs), modes=modes, **arena.outputs(given))
    return arena.read(given)


def _max_boundary(refs, un, w, h):
    """Largest boundary or corner sample of the available CUs of refs [H, W]."""
    _, x, y, bw, bh = layout.cu_geometry(w, h, np.arange(un.size))
    best = 0
    for s in layout.SHAPES:
        k = np.nonzero(~un & (bw == s.w) & (bh == s.h))[0]
        if k.size:
            top, left, corner = A.boundaries(refs, x[k], y[k], s.w, s.h)
            best = max(best, int(top.max()), int(left.max()), int(corner.max()))
    return best


@pytest.mark.parametrize("filt", (None, FILTER), ids=("orig", "1d_int"))
def test_full_tables_device_and_host(gpu_available, filt):
    """136x72: two CTU columns, partial CTUs right and below, wrapped CUs.  All 3 x 2 x 5380 x 65
    entries of every table and the ang pair, device and host call."""
    w, h = 136, 72
    frames, refs, un, ref = AC.case(w, h, filt)
    _, x, y, _, _ = layout.cu_geometry(w, h, np.arange(un.size))
    ok = ~un
    assert (ok & (x == 0) & (y == 0)).any() and (ok & (x == 0) & (y > 0)).any() and (ok & (y == 0) & (x > 0)).any()
    assert (ok & (x + 4 > w)).any()                           # CUs right of the frame (wrapped samples)
    if filt is not None:                                      # 32-bit arithmetic and the clip are exercised
        assert max(_max_boundary(r, un, w, h) for r in refs) > 1023
    with MipEngine(w, h, filter=filt, max_batch=3) as eng:
        got, clean = _run(eng, frames)
        host = eng.angular(frames, table=True)
        pair_only = eng.angular(frames[1:])
    assert clean
    for key in ALL_OUT:
        assert np.array_equal(got[key], ref[key]), key
    for key in ("cost", "ang_mode", "ang_cost"):
        assert np.array_equal(host[key], ref[key]), key
    for key in AC.TABLES:
        assert np.array_equal(got[key][:, :, 0] == UN, np.broadcast_to(un, got[key].shape[:2])), key
    assert sorted(pair_only) == ["ang_cost", "ang_mode"] and np.array_equal(pair_only["ang_mode"], ref["ang_mode"][1:])
    assert np.array_equal(pair_only["ang_cost"], ref["ang_cost"][1:])
    assert np.array_equal(got["cost"], np.where(got["sad"] == UN, UN, np.minimum(2 * got["sad"].astype(np.int64), got["satd"])))
    assert np.all(got["ang_mode"][:, un] == 0xFF) and np.all(got["ang_cost"][:, un] == UN)
    assert len(np.unique(got["ang_mode"])) > 40               # most modes win somewhere


@pytest.mark.parametrize("modes, given", [((18, 34, 50), ALL_OUT), (AC.EVEN_MODES, ("cost", "ang_mode", "ang_cost")), ((23,), ("sad",)),
                                          ((23,), ("satd", "ang_mode", "ang_cost"))],
                         ids=("pure+diagonal", "even", "single-sad", "single-satd+pair"))
def test_mode_lists_and_outputs_not_asked_for(gpu_available, modes, given):
    """Slots of modes not in the list are MIP_COST_UNAVAILABLE, listed slots are the all-modes
    values, the best is taken over the list; outputs that were not passed are not written."""
    w, h = 136, 72
    frames, _, un, full = AC.case(w, h, None)
    listed = np.zeros(65, bool)
    listed[np.array(modes) - 2] = True
    with MipEngine(w, h, max_batch=3) as eng:
        got, clean = _run(eng, frames, modes=modes, given=given)
    assert clean
    for key in given:
        if key in AC.TABLES:
            assert np.array_equal(got[key][..., listed], full[key][..., listed]), key
            assert np.all(got[key][..., ~listed] == UN), key
    if "ang_cost" in given:
        want_mode, want_cost = A.best(np.where(listed, full["cost"], UN))
        assert np.array_equal(got["ang_mode"], want_mode) and np.array_equal(got["ang_cost"], want_cost)
        assert set(np.unique(want_mode)) == {0x80 + m for m in modes} | {0xFF}


def test_structured_frames(gpu_available):
    """f(x), f(y) and f(x - y) as three frames of one call: modes 50, 18 and 34 predict every
    interior CU exactly (tests/test_angular_cpu.py says which CUs), and win."""
    w, h = 136, 72
    frames = np.stack([AC.structured(k, w, h) for k in ("x", "y", "x-y")])
    un = mipgpu.unavailable_cus(w, h)
    _, x, y, bw, _ = layout.cu_geometry(w, h, np.arange(un.size))
    inner = ~un & (x > 0) & (y > 0)
    with MipEngine(w, h, max_batch=3) as eng:
        got, clean = _run(eng, frames, given=("ang_mode", "ang_cost"))
    assert clean
    for f, (mode, cus) in enumerate(((50, inner), (18, inner & (x + bw <= w)), (34, inner & (x + bw <= w)))):
        assert cus.sum() > 1000
        assert np.all(got["ang_mode"][f, cus] == 0x80 + mode) and not got["ang_cost"][f, cus].any(), mode
    want = [A.best(A.tables(f, f, un)["cost"]) for f in frames]
    assert np.array_equal(got["ang_mode"], np.stack([m for m, _ in want])) and np.array_equal(got["ang_cost"], np.stack([c for _, c in want]))


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
    frames, _, un, ref = AC.case(w, h, None)
    even_mode, even_cost = A.best(np.where(np.arange(65) % 2 == 0, ref["cost"], UN))
    with MipEngine(w, h, max_batch=3) as eng:
        d_frames = _dev(frames)
        bm, bc = _decisions(eng, d_frames)
        bm0, bc0 = bm.cpu().numpy(), bc.cpu().numpy()
        assert np.array_equal(bc0 == UN, np.broadcast_to(un, bc0.shape)) and np.all(bm0[bc0 == UN] == 0xFF)
        taken = []
        for bias in (0, 300, 1 << 20):
            m, c = bm.clone(), bc.clone()
            assert eng.angular_device(d_frames, bias=bias, best_mode=m, best_cost=c) is None   # merge only
            wm, wc = A.merge(bm0, bc0, ref["ang_mode"], ref["ang_cost"], bias)
            assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(c.cpu().numpy(), wc), bias
            assert np.array_equal(wm[:, un], bm0[:, un])
            taken.append(int(((wm >= 0x82) & (wm <= 0xC2)).sum()))
            assert ((wm < 32) & ~un).any()                    # MIP decisions survive
        assert taken[0] > taken[1] > taken[2] and taken[2] < taken[0] // 100   # the bias decides
        # after a Planar / DC merge: the chain intra_device -> angular_device, with the even modes,
        # tables and the ang pair in the same call
        m, c = bm.clone(), bc.clone()
        eng.intra_device(d_frames, bias=(20, 20), best_mode=m, best_cost=c)
        pm, pc = m.cpu().numpy(), c.cpu().numpy()
        assert ((pm == mipgpu.MODE_PLANAR) | (pm == mipgpu.MODE_DC)).any()
        arena = Arena(3, eng.cus_per_frame)
        eng.angular_device(d_frames, modes=AC.EVEN_MODES, bias=40, best_mode=m, best_cost=c, **arena.outputs(("cost", "ang_mode", "ang_cost")))
        got, clean = arena.read(("cost", "ang_mode", "ang_cost"))
        wm, wc = A.merge(pm, pc, even_mode, even_cost, 40)
        assert clean and np.array_equal(got["ang_mode"], even_mode) and np.array_equal(got["ang_cost"], even_cost)
        assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(c.cpu().numpy(), wc)
        kinds = [(wm < 32) & ~un, (wm == mipgpu.MODE_PLANAR) | (wm == mipgpu.MODE_DC), (wm >= 0x82) & (wm <= 0xC2)]
        assert all(k.any() for k in kinds)                    # MIP, Planar / DC and angular decisions all survive
        # a bias outside 0 .. 1<<20 or a bad list is refused before any launch, nothing written
        arena = Arena(3, eng.cus_per_frame)
        for bad in (dict(bias=-1), dict(bias=(1 << 20) + 1), dict(modes=(20, 20)), dict(modes=(21, 20)), dict(modes=(1, 2)),
                    dict(modes=(66, 67)), dict(modes=()), dict(modes=tuple(range(1, 67)))):
            m, c = bm.clone(), bc.clone()
            with pytest.raises(mipgpu.MipError, match="bias" if "bias" in bad else "modes"):
                eng.angular_device(d_frames, best_mode=m, best_cost=c, **arena.outputs(ALL_OUT), **bad)
            torch.cuda.synchronize()
            assert torch.equal(m, bm) and torch.equal(c, bc), bad
        assert arena.read(())[1]
        for half in (dict(best_cost=bc.clone()), dict(ang_mode=arena.tensor("ang_mode"))):
            with pytest.raises(mipgpu.MipError, match="together"):
                eng.angular_device(d_frames, **half)
        s = torch.cuda.current_stream()                       # no output at all
        rc = mipgpu.library().mip_angular_device(eng._h, d_frames.data_ptr(), None, 3, None, 0, None, None, None, None, None, 0, None,
                                                 None, ctypes.c_void_p(s.cuda_stream))
        assert rc != 0 and "no output" in mipgpu.library().mip_last_error().decode()
        assert arena.read(())[1]


def test_merge_ties_on_a_uniform_frame(gpu_available):
    """Uniform frame: every angular mode costs 0 away from the frame's first row and column, so
    the best is the first mode of the list.  Constant decisions of cost 5: bias 5 ties and the
    decision stays (strictly lower only), bias 4 undercuts by 1 and the angular mode is taken;
    unavailable CUs are untouched."""
    w, h = 136, 72
    frame = np.full((1, h, w), 700, np.uint16)
    un = mipgpu.unavailable_cus(w, h)
    _, x, y, _, _ = layout.cu_geometry(w, h, np.arange(un.size))
    flat = ~un & (x > 0) & (y > 0)
    five = np.where(un, UN, 5).astype(np.int32)[None]
    mode5 = np.where(un, 0xFF, 1).astype(np.uint8)[None]
    with MipEngine(w, h) as eng:
        d_frames = _dev(frame)
        for modes, first in ((None, 2), ((31, 50, 64), 31)):
            ref_mode, ref_cost = A.best(A.tables(frame[0], frame[0], un, modes)["cost"][None])
            assert np.all(ref_mode[0, ~un] == 0x80 + first) and not ref_cost[0, flat].any()
            for bias, want in ((5, 1), (4, 0x80 + first), (0, 0x80 + first), (6, 1)):
                m, c = _dev(mode5), _dev(five)
                eng.angular_device(d_frames, modes=modes, bias=bias, best_mode=m, best_cost=c)
                wm, wc = A.merge(mode5, five, ref_mode, ref_cost, bias)
                assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(c.cpu().numpy(), wc), (modes, bias)
                assert np.all(wm[0, flat] == want) and np.all(wc[0, flat] == (5 if want == 1 else bias)), (modes, bias)
                assert np.all(wm[0, un] == 0xFF) and np.all(wc[0, un] == UN)


def test_merged_decisions_feed_partition_and_prediction(gpu_available):
    import torch
    w, h, penalty = 136, 72, 600
    frames = AC.C.frames(w, h)[:1]
    with MipEngine(w, h) as eng:
        d_frames = _dev(frames)
        bm, bc = _decisions(eng, d_frames)
        eng.intra_device(d_frames, bias=(30, 30), best_mode=bm, best_cost=bc)
        eng.angular_device(d_frames, bias=60, best_mode=bm, best_cost=bc)
        nct = eng.nctus
        items = torch.zeros((1, nct, mipgpu.PART_MAX_LEAVES * mipgpu.PRED_ITEM.itemsize), dtype=torch.uint8, device="cuda")
        ctu_cost = torch.zeros((1, nct), dtype=torch.int32, device="cuda")
        ctu_leaves = torch.zeros((1, nct), dtype=torch.int32, device="cuda")
        leaf = torch.zeros((1, eng.cus_per_frame), dtype=torch.uint8, device="cuda")
        mipgpu.partition_device(bc, w, h, penalty=penalty, best_mode=bm, leaf=leaf, ctu_cost=ctu_cost, ctu_leaves=ctu_leaves,
                                items=items)
        canvas = torch.full((w * h,), -1, dtype=torch.int16, device="cuda")
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.predict_device(d_frames, items, canvas, skipped=sk, regular=True)
        eng.check_input()
        torch.cuda.synchronize()
    mode, cost, leaf = bm.cpu().numpy(), bc.cpu().numpy(), leaf.cpu().numpy().astype(bool)
    ref = R.partition_frames(cost, w, h, penalty)
    assert np.array_equal(ctu_cost.cpu().numpy(), ref["ctu_cost"]) and np.array_equal(leaf, ref["leaf"].astype(bool))
    assert np.array_equal(ctu_leaves.cpu().numpy()[0], leaf[0].reshape(nct, -1).sum(axis=1))
    angular = leaf & (mode >= 0x82) & (mode <= 0xC2)
    assert angular.any() and (leaf & ~angular).any()          # leaves of both kinds
    padding = nct * mipgpu.PART_MAX_LEAVES - int(ctu_leaves.sum().item())
    assert int(sk.item()) == padding + int(angular.sum())     # exactly the padding and the angular leaves are skipped
    # the angular leaves' samples stay unwritten, the MIP, Planar and DC leaves' are predicted
    got = canvas.cpu().numpy().view(np.uint16).reshape(h, w)
    _, x, y, bw, bh = layout.cu_geometry(w, h, np.nonzero(leaf[0])[0])
    for k, cu in enumerate(np.nonzero(leaf[0])[0]):
        blk = got[y[k]:y[k] + bh[k], x[k]:x[k] + bw[k]]
        assert np.all(blk == 0xFFFF) if angular[0, cu] else np.all(blk <= 1023), int(cu)


def test_second_geometry_two_frames(gpu_available):
    """264x136, two frames in one call: frame indexing and a CTU grid of more than one row; five
    modes of both classes and both angle signs."""
    w, h, modes = 264, 136, (5, 18, 30, 41, 60)
    assert [A.ANGLE[m] > 0 for m in (5, 30, 41, 60)] == [True, False, False, True]
    frames, _, un, ref = AC.case(w, h, None, 2, modes)
    assert layout.ctu_grid(w, h) == (3, 2)
    with MipEngine(w, h, max_batch=2) as eng:
        got, clean = _run(eng, frames, modes=modes)
    assert clean
    for key in ALL_OUT:
        assert np.array_equal(got[key], ref[key]), key
    assert not np.array_equal(got["ang_cost"][0], got["ang_cost"][1])


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
    """The kernel stages frames and references with 2-byte loads: frames, and frames plus caller
    references, at an odd sample offset give the results of the aligned call."""
    w, h, modes = 136, 72, (9, 26, 34, 58)
    frames, _, un, full = AC.case(w, h, None)
    caller = frames[::-1]                                     # another frame's samples as references
    want = [A.tables(f, r, un, modes) for f, r in zip(frames[:2], caller[:2])]
    listed = np.zeros(65, bool)
    listed[np.array(modes) - 2] = True
    with MipEngine(w, h, max_batch=3) as eng:
        arena = Arena(3, eng.cus_per_frame)
        eng.angular_device(_odd_view(frames), modes=modes, **arena.outputs(ALL_OUT))
        got, clean = arena.read(ALL_OUT)
        arena_r = Arena(2, eng.cus_per_frame)
        eng.angular_device(_odd_view(frames[:2]), modes=modes, refs=_odd_view(caller[:2]), **arena_r.outputs(ALL_OUT))
        got_r, clean_r = arena_r.read(ALL_OUT)
    assert clean and clean_r
    for key in AC.TABLES:
        assert np.array_equal(got[key], np.where(listed, full[key], UN)), key
        assert np.array_equal(got_r[key], np.stack([t[key] for t in want])), key
    wm, wc = A.best(got_r["cost"])
    assert np.array_equal(got_r["ang_mode"], wm) and np.array_equal(got_r["ang_cost"], wc)
    assert not np.array_equal(got_r["cost"], got["cost"][:2])


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_multipass(gpu_available):
    """2 1/3 rounds of the launcher's capped grid at 136x72 (2 CTUs, 40 items per frame), four
    modes, the cost table, the ang pair and the merge in one launch.  A workgroup's item index
    inside the CTU moves by cap % 20 per pass, so workgroups go from a 64x64 item to a 32x32 one
    and back and reuse their LDS window (and the 64x64 CU's per-mode sums) for an item of the other
    kind.  The frames repeat with period 3; the table is compared on the device."""
    import torch
    import launch_caps as L
    w, h, modes, bias = 136, 72, (3, 18, 40, 66), 9
    frames, _, un, ref = AC.case(w, h, None, 3, modes)
    unit = layout.num_ctus(w, h) * AC.ANGULAR_ITEMS_PER_CTU
    cap = AC.angular_cap(_cus())
    nframes = -(-L.multipass_work(cap) // unit)
    assert L.passes(nframes * unit, cap) == (2, 3)
    k0, k1 = np.arange(cap) % AC.ANGULAR_ITEMS_PER_CTU, (np.arange(cap) + cap) % AC.ANGULAR_ITEMS_PER_CTU
    big0, big1 = k0 < AC.ANGULAR_BIG_ITEMS, k1 < AC.ANGULAR_BIG_ITEMS
    assert cap % AC.ANGULAR_ITEMS_PER_CTU and (big0 & ~big1).any() and (~big0 & big1).any()
    assert cap % (3 * unit)                                   # the content's period does not divide the grid
    sel = np.arange(nframes) % 3
    rng = np.random.default_rng(nframes)
    near = np.where(ref["ang_cost"] == UN, 0, ref["ang_cost"])[sel]
    best_cost = (near + rng.integers(-40, 41, near.shape) * rng.integers(0, 2, near.shape)).clip(0).astype(np.int32)
    best_mode = rng.integers(0, 12, best_cost.shape).astype(np.uint8)
    dead = np.broadcast_to(un, best_cost.shape) | (rng.random(best_cost.shape) < 0.05)
    best_cost[dead], best_mode[dead] = UN, 0xFF
    with MipEngine(w, h, max_batch=nframes) as eng:
        ncu = eng.cus_per_frame
        cost = torch.full((nframes, ncu, 65), -7, dtype=torch.int32, device="cuda")
        am = torch.full((nframes, ncu), 0x5A, dtype=torch.uint8, device="cuda")
        ac = torch.full((nframes, ncu), -7, dtype=torch.int32, device="cuda")
        m, c = _dev(best_mode), _dev(best_cost)
        eng.angular_device(_dev(frames[sel]), modes=modes, cost=cost, ang_mode=am, ang_cost=ac, bias=bias, best_mode=m, best_cost=c)
        want = _dev(ref["cost"])
        for f0 in range(0, nframes, 48):                      # (48 frames = 16 periods)
            part = cost[f0:f0 + 48]
            same = part == want[torch.from_numpy(sel[f0:f0 + 48]).cuda()]
            assert bool(same.all()), (f0, torch.nonzero(~same)[:4].cpu().numpy())
        got_am, got_ac, got_m, got_c = am.cpu().numpy(), ac.cpu().numpy(), m.cpu().numpy(), c.cpu().numpy()
    assert np.array_equal(got_am, ref["ang_mode"][sel]) and np.array_equal(got_ac, ref["ang_cost"][sel])
    want_mode, want_cost = A.merge(best_mode, best_cost, ref["ang_mode"][sel], ref["ang_cost"][sel], bias)
    assert np.array_equal(got_m, want_mode) and np.array_equal(got_c, want_cost)
    assert (want_mode >= 0x82).any() and (want_mode < 12).any() and np.array_equal(want_mode[dead], best_mode[dead])


def test_chunked_host_call_equals_the_device_call(gpu_available):
    """The host call of 3 frames on max_batch = 2 runs two chunks; caller references equal to the
    oracle-filtered frames give the engine-filter result on every CU available in both sets."""
    w, h = 136, 72
    frames, refs, un_f, ref_f = AC.case(w, h, FILTER)
    un_o = mipgpu.unavailable_cus(w, h)
    both = ~un_f & ~un_o
    assert both.any() and (un_f & ~un_o).any()
    with MipEngine(w, h, max_batch=2) as eng:
        got, clean = _run(eng, frames[:2], refs=refs[:2], given=("cost", "ang_mode", "ang_cost"))
        host = eng.angular(frames, refs=refs, table=True)
        with pytest.raises(mipgpu.MipError, match="modes"):
            eng.angular(frames, modes=(4, 3))
    assert clean
    for key in ("cost", "ang_mode", "ang_cost"):
        assert np.array_equal(got[key][:, both], ref_f[key][:2][:, both]), key
        assert np.array_equal(host[key][:, both], ref_f[key][:, both]), key
        assert np.array_equal(host[key][:2], got[key]), key
    assert np.array_equal(host["ang_cost"] == UN, np.broadcast_to(un_o, host["ang_cost"].shape))


def test_angular_and_search_share_the_filter_scratch_on_two_streams(gpu_available):
    """angular_device on one stream and search_device on another, both filtering into the engine's
    reference scratch (no caller references), different frames, four alternating rounds: each
    launch waits for the previous reader of the scratch, so each gives its own references'
    result.  More frames than max_batch are refused on a filtering engine."""
    import torch
    import oracle_lib as O
    from mipgpu.synth import synth_frames
    w, h, modes = 136, 72, (2, 34, 50, 61)
    frames, _, un, ref = AC.case(w, h, FILTER)
    listed = np.zeros(65, bool)
    listed[np.array(modes) - 2] = True
    want_cost = np.where(listed, ref["cost"], UN)
    other = synth_frames(w, h, 2, 0x2B7, 0)
    want = np.stack([O.engine_search(f, FILTER, 0) for f in other])
    rounds = 4
    with MipEngine(w, h, filter=FILTER, max_batch=3) as eng:
        d_ang = [_dev(np.roll(frames, -i, axis=0)) for i in range(3)]
        d_search = [_dev(other[::s]) for s in (1, -1)]
        arenas = [Arena(3, eng.cus_per_frame) for _ in range(rounds)]
        costs = [torch.full((2, eng.costs_per_frame), -7, dtype=torch.int32, device="cuda") for _ in range(rounds)]
        torch.cuda.synchronize()                              # inputs and prefills ran on the current stream
        s_ang, s_search = torch.cuda.Stream(), torch.cuda.Stream()
        for i in range(rounds):
            eng.angular_device(d_ang[i % 3], modes=modes, stream=s_ang, **arenas[i].outputs(("cost", "ang_mode", "ang_cost")))
            eng.search_device(d_search[i % 2], costs=costs[i], stream=s_search)
        torch.cuda.synchronize()
        eng.check_input(stream=s_search)
        for i in range(rounds):
            got, clean = arenas[i].read(("cost", "ang_mode", "ang_cost"))
            assert clean, i
            assert np.array_equal(got["cost"], np.roll(want_cost, -(i % 3), axis=0)), i
            assert np.array_equal(got["ang_cost"], A.best(got["cost"])[1]), i
            assert np.array_equal(costs[i].cpu().numpy(), want[::1 if i % 2 == 0 else -1]), i
    with MipEngine(w, h, filter=FILTER, max_batch=2) as eng:
        arena = Arena(3, eng.cus_per_frame)
        with pytest.raises(mipgpu.MipError, match="max_batch"):
            eng.angular_device(_dev(frames), **arena.outputs(ALL_OUT))
        assert arena.read(())[1]
