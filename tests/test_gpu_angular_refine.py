"""Coarse-to-fine angular search on the GPU (mip_angular_refine_device /
mip_angular_refine_frames): tables, ang pair, `tried` and both merges equal the numpy restatement
(tests/angular_refine_ref.py, pinned by tests/test_angular_refine_cpu.py) bit for bit for the
lists even, odd, (2, 34, 66) and all 65 with one, two and three seeds; calls with one output give
the same values and write nothing else; the structured frames reach modes 18, 34 and 50 through
their neighbours; 2 1/3 rounds of the capped grid; the host call across a chunk boundary; and the
device chain search -> Planar / DC merge -> refined angular merge -> partition -> prediction."""
import numpy as np
import pytest

import angular_cases as AC
import angular_ref as A
import angular_refine_cases as RC
import angular_refine_ref as RR
import edge_sweep_cases as E
import mipgpu
import partition_ref as R
from mipgpu import MipEngine, layout

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements before and after every output
GUARD_WORD, GUARD_BYTE = -0x5A5A5A5B, 0x5A
UN = layout.UNAVAILABLE
INT32_OUT = AC.TABLES + ("ang_cost",)
BYTE_OUT = ("ang_mode", "tried")
ALL_OUT = INT32_OUT + BYTE_OUT


def _dev(a):
    import torch
    a = np.array(a, copy=True)                               # (the shared cases are read-only)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


class Arena:
    """The three tables and ang_cost inside one guard-filled int32 device buffer, ang_mode and
    tried inside a guard-filled uint8 one, so that a write outside an output -- or into one that
    was not passed -- shows."""

    def __init__(self, nframes, ncu, keys=ALL_OUT):
        import torch
        self.size = {k: nframes * ncu * (65 if k in AC.TABLES else 1) for k in keys}
        self.shape = {k: (nframes, ncu, 65) if k in AC.TABLES else (nframes, ncu) for k in keys}
        self.at, end = {}, GUARD
        for k in (k for k in INT32_OUT if k in keys):
            self.at[k], end = end, end + self.size[k] + GUARD
        self.buf = torch.full((end,), GUARD_WORD, dtype=torch.int32, device="cuda")
        end = GUARD
        for k in (k for k in BYTE_OUT if k in keys):
            self.at[k], end = end, end + self.size[k] + GUARD
        self.bytes = torch.full((end,), GUARD_BYTE, dtype=torch.uint8, device="cuda")

    def tensor(self, key):
        src = self.bytes if key in BYTE_OUT else self.buf
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
            host, clean = (octets, clean_b) if key in BYTE_OUT else (words, clean_w)
            clean[self.at[key]:self.at[key] + self.size[key]] = False
            out[key] = host[self.at[key]:self.at[key] + self.size[key]].reshape(self.shape[key])
        return out, bool(np.all(words[clean_w] == GUARD_WORD) and np.all(octets[clean_b] == GUARD_BYTE))


def _decisions(eng, d_frames):
    import torch
    n = d_frames.shape[0]
    bm = torch.full((n, eng.cus_per_frame), 0x5A, dtype=torch.uint8, device="cuda")
    bc = torch.full((n, eng.cus_per_frame), -3, dtype=torch.int32, device="cuda")
    eng.search_device(d_frames, costs=False, best_mode=bm, best_cost=bc)
    return bm, bc


@pytest.mark.parametrize("name", list(RC.LISTS))
@pytest.mark.parametrize("geometry", RC.GEOMETRIES, ids=lambda g: "%dx%d-%s" % (g[0], g[1], "orig" if g[2] is None else "1d_int"))
def test_everything_equals_the_restatement(gpu_available, geometry, name):
    """Three frames, one list, seeds 1..3: every table, the ang pair, `tried`, the merge into the
    search's decisions (in the same call) and into decisions already merged by intra_device (a
    call with the merge pair only), and a call with `tried` only."""
    import torch
    w, h, filt = geometry
    frames, _, un, full = AC.case(w, h, filt)
    modes = RC.LISTS[name]
    with MipEngine(w, h, filter=filt, max_batch=3) as eng:
        d_frames = _dev(frames)
        bm, bc = _decisions(eng, d_frames)
        im, ic = bm.clone(), bc.clone()
        eng.intra_device(d_frames, bias=(20, 20), best_mode=im, best_cost=ic)
        bm0, bc0, im0, ic0 = (t.cpu().numpy() for t in (bm, bc, im, ic))
        assert np.array_equal(bc0 == UN, np.broadcast_to(un, bc0.shape)) and (im0 >= mipgpu.MODE_PLANAR).any()
        for seeds in RC.SEEDS:
            want = RC.refined(w, h, filt, name, seeds)
            arena = Arena(3, eng.cus_per_frame)
            m, c = bm.clone(), bc.clone()
            assert eng.angular_refine_device(d_frames, modes=modes, seeds=seeds, bias=9, best_mode=m, best_cost=c,
                                             **arena.outputs(ALL_OUT)) is None
            got, clean = arena.read(ALL_OUT)
            assert clean, seeds
            for key in ALL_OUT:
                assert np.array_equal(got[key], want[key]), (seeds, key)
            wm, wc = A.merge(bm0, bc0, want["ang_mode"], want["ang_cost"], 9)
            assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(c.cpu().numpy(), wc), seeds
            # the merge pair only, on decisions that hold Planar / DC
            arena = Arena(3, eng.cus_per_frame)
            m, c = im.clone(), ic.clone()
            eng.angular_refine_device(d_frames, modes=modes, seeds=seeds, bias=40, best_mode=m, best_cost=c)
            wm, wc = A.merge(im0, ic0, want["ang_mode"], want["ang_cost"], 40)
            assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(c.cpu().numpy(), wc), seeds
            assert np.array_equal(wm[:, un], im0[:, un])
            # `tried` only
            eng.angular_refine_device(d_frames, modes=modes, seeds=seeds, tried=arena.tensor("tried"))
            got, clean = arena.read(("tried",))
            assert clean and np.array_equal(got["tried"], want["tried"]), seeds
            if name == "all":                                 # no candidates: mip_angular_device's outputs
                assert np.array_equal(want["ang_mode"], full["ang_mode"]) and np.all(want["tried"][:, ~un] == 65)
            else:
                assert (want["ang_cost"] < A.best(np.where(RR.listed_mask(modes), full["cost"], UN))[1]).any()
        torch.cuda.synchronize()


def test_argument_rules(gpu_available):
    """seeds outside 1..3, a bad list, a bad bias, half a pair and no output are refused before
    any launch: nothing is written."""
    import ctypes
    import torch
    w, h = 60, 36
    frames = AC.case(w, h, None)[0]
    with MipEngine(w, h, max_batch=3) as eng:
        d_frames = _dev(frames)
        bm, bc = _decisions(eng, d_frames)
        arena = Arena(3, eng.cus_per_frame)
        for bad, text in ((dict(seeds=0), "seeds"), (dict(seeds=4), "seeds"), (dict(seeds=-1), "seeds"), (dict(bias=-1), "bias"),
                          (dict(bias=(1 << 20) + 1), "bias"), (dict(modes=(20, 20)), "modes"), (dict(modes=(1, 2)), "modes")):
            m, c = bm.clone(), bc.clone()
            with pytest.raises(mipgpu.MipError, match=text):
                eng.angular_refine_device(d_frames, best_mode=m, best_cost=c, **arena.outputs(ALL_OUT), **bad)
            torch.cuda.synchronize()
            assert torch.equal(m, bm) and torch.equal(c, bc), bad
        for half in (dict(best_cost=bc.clone()), dict(ang_mode=arena.tensor("ang_mode"))):
            with pytest.raises(mipgpu.MipError, match="together"):
                eng.angular_refine_device(d_frames, **half)
        s = torch.cuda.current_stream()
        rc = mipgpu.library().mip_angular_refine_device(eng._h, d_frames.data_ptr(), None, 3, None, 0, 1, None, None, None, None, None,
                                                        None, 0, None, None, ctypes.c_void_p(s.cuda_stream))
        assert rc != 0 and "no output" in mipgpu.library().mip_last_error().decode()
        with pytest.raises(mipgpu.MipError, match="seeds"):
            eng.angular_refine(frames, seeds=4)
        assert arena.read(())[1]


def test_structured_frames_reach_their_mode(gpu_available):
    """f(x), f(y), f(x - y) as three frames of one call with the odd list: 50, 18 and 34 are not in
    it and win as candidates (PDPC and the exact diagonal as per-lane modes) wherever the best odd
    mode is their neighbour (tests/test_angular_refine_cpu.py counts the few CUs where it is not)."""
    w, h = 136, 72
    frames = np.stack([AC.structured(k, w, h) for k, _ in RC.STRUCTURED])
    un = mipgpu.unavailable_cus(w, h)
    _, x, y, bw, _ = layout.cu_geometry(w, h, np.arange(un.size))
    inner = ~un & (x > 0) & (y > 0)
    full = {k: np.stack([A.tables(f, f, un)[k] for f in frames]) for k in AC.TABLES}
    for seeds in (1, 3):
        want = RR.refine(full, RR.ODD_MODES, seeds)
        with MipEngine(w, h, max_batch=3) as eng:
            arena = Arena(3, eng.cus_per_frame)
            eng.angular_refine_device(_dev(frames), modes=RR.ODD_MODES, seeds=seeds, **arena.outputs(ALL_OUT))
            got, clean = arena.read(ALL_OUT)
        assert clean
        for key in ALL_OUT:
            assert np.array_equal(got[key], want[key]), (seeds, key)
        for f, (kind, mode) in enumerate(RC.STRUCTURED):
            cus = inner & (x + bw <= w if kind != "x" else True) & np.isin(want["seeds"][f, :, 0], (mode - 1, mode + 1))
            assert cus.sum() > 2500 and np.all(got["ang_mode"][f, cus] == 0x80 + mode) and not got["ang_cost"][f, cus].any(), kind


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_multipass(gpu_available):
    """2 1/3 rounds of the launcher's capped grid at 128x128 (one whole CTU, 20 items per frame):
    the even list, two seeds, the ang pair, `tried` and the merge in one launch.  A workgroup's
    item index inside the CTU moves by cap % 20 per pass, so workgroups go from a 64x64 item to a
    32x32 one and back and reuse their LDS window, the waves' sums and the candidate cells for an
    item of the other kind.  The frames repeat with period 3."""
    import launch_caps as L
    w, h, bias, seeds = 128, 128, 9, 2
    frames, _, un, full = AC.case(w, h, None)
    want = RR.refine({k: full[k] for k in AC.TABLES}, RR.EVEN_MODES, seeds)
    unit = layout.num_ctus(w, h) * AC.ANGULAR_ITEMS_PER_CTU
    cap = AC.angular_cap(_cus())
    nframes = -(-L.multipass_work(cap) // unit)
    assert unit == 20 and L.passes(nframes * unit, cap) == (2, 3)
    k0, k1 = np.arange(cap) % AC.ANGULAR_ITEMS_PER_CTU, (np.arange(cap) + cap) % AC.ANGULAR_ITEMS_PER_CTU
    big0, big1 = k0 < AC.ANGULAR_BIG_ITEMS, k1 < AC.ANGULAR_BIG_ITEMS
    assert cap % AC.ANGULAR_ITEMS_PER_CTU and (big0 & ~big1).any() and (~big0 & big1).any()
    sel = np.arange(nframes) % 3
    rng = np.random.default_rng(nframes)
    near = np.where(want["ang_cost"] == UN, 0, want["ang_cost"])[sel]
    best_cost = (near + rng.integers(-40, 41, near.shape) * rng.integers(0, 2, near.shape)).clip(0).astype(np.int32)
    best_mode = rng.integers(0, 12, best_cost.shape).astype(np.uint8)
    dead = np.broadcast_to(un, best_cost.shape) | (rng.random(best_cost.shape) < 0.05)
    best_cost[dead], best_mode[dead] = UN, 0xFF
    with MipEngine(w, h, max_batch=nframes) as eng:
        given = ("ang_mode", "ang_cost", "tried")
        arena = Arena(nframes, eng.cus_per_frame, given)
        m, c = _dev(best_mode), _dev(best_cost)
        eng.angular_refine_device(_dev(frames[sel]), modes=RR.EVEN_MODES, seeds=seeds, bias=bias, best_mode=m, best_cost=c,
                                  **arena.outputs(given))
        got, clean = arena.read(given)
        got_m, got_c = m.cpu().numpy(), c.cpu().numpy()
    assert clean
    for key in given:
        assert np.array_equal(got[key], want[key][sel]), key
    want_mode, want_cost = A.merge(best_mode, best_cost, want["ang_mode"][sel], want["ang_cost"][sel], bias)
    assert np.array_equal(got_m, want_mode) and np.array_equal(got_c, want_cost)
    assert (want_mode >= 0x82).any() and (want_mode < 12).any() and np.array_equal(want_mode[dead], best_mode[dead])
    assert (want["tried"] > 33).any() and (want["ang_mode"].astype(int) % 2 == 1).any()   # odd modes win somewhere


def test_host_call_equals_the_device_call_across_a_chunk_boundary(gpu_available):
    w, h, seeds = 136, 72, 2
    frames, _, un, _ = AC.case(w, h, None)
    want = RC.refined(w, h, None, "even", seeds)
    with MipEngine(w, h, max_batch=3) as eng:
        arena = Arena(3, eng.cus_per_frame)
        eng.angular_refine_device(_dev(frames), modes=RR.EVEN_MODES, seeds=seeds, **arena.outputs(ALL_OUT))
        got, clean = arena.read(ALL_OUT)
        whole = eng.angular_refine(frames, modes=mipgpu.ANGULAR_EVEN_MODES, seeds=seeds, table=True)
    with MipEngine(w, h, max_batch=2) as eng:                 # chunks of 2 and 1 frames
        cut = eng.angular_refine(frames, modes=mipgpu.ANGULAR_EVEN_MODES, seeds=seeds, table=True)
        pair = eng.angular_refine(frames, modes=mipgpu.ANGULAR_EVEN_MODES, seeds=seeds)
        caller = eng.angular_refine(frames, refs=frames, modes=mipgpu.ANGULAR_EVEN_MODES, seeds=seeds)
    assert clean and sorted(whole) == ["ang_cost", "ang_mode", "cost", "tried"] and sorted(pair) == ["ang_cost", "ang_mode", "tried"]
    for key in ("cost", "ang_mode", "ang_cost", "tried"):
        assert np.array_equal(got[key], want[key]), key
        assert np.array_equal(whole[key], got[key]) and np.array_equal(cut[key], got[key]), key
    for key in ("ang_mode", "ang_cost", "tried"):
        assert np.array_equal(pair[key], got[key]) and np.array_equal(caller[key], got[key]), key


def test_device_chain(gpu_available):
    """search_device -> intra_device -> angular_refine_device (even list, one seed) ->
    partition_device -> predict_device(regular=True, angular=True) at 136x72: leaves and CTU costs
    are the restatement's chain's (the C oracle's argmin, tests/intra_ref.py's merge, the refined
    pair's merge, tests/partition_ref.py), nothing but the list's padding is skipped, partitioned
    CTUs have no hole and every angular leaf's block is angular_ref.predict's."""
    import torch
    from test_gpu_predict_angular import BASE, FILL, _host, _is_angular, _leaf_blocks, _sentinel
    w, h = 136, 72
    c = E.chain_case(w, h)
    frame, _, un, tabs = E.angular_sweep_case(w, h, "edges", None, None)
    assert np.array_equal(frame, c["frame"])
    fine = RR.refine({k: tabs[k][None] for k in AC.TABLES}, RR.EVEN_MODES, 1)
    mode, cost = A.merge(c["best_mode"], c["best_cost"], fine["ang_mode"], fine["ang_cost"], E.ANGULAR_CHAIN_BIAS)
    ref = R.partition_frames(cost, w, h, E.CHAIN_PENALTY, best_mode=mode)
    with MipEngine(w, h) as eng:
        nct, ncu = eng.nctus, eng.cus_per_frame
        d_frames = _dev(frame[None])
        bm, bc = _decisions(eng, d_frames)
        eng.intra_device(d_frames, bias=E.CHAIN_BIAS, best_mode=bm, best_cost=bc)
        eng.angular_refine_device(d_frames, modes=mipgpu.ANGULAR_EVEN_MODES, seeds=1, bias=E.ANGULAR_CHAIN_BIAS, best_mode=bm, best_cost=bc)
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
    got_mode, got_cost = bm.cpu().numpy(), bc.cpu().numpy()
    assert np.array_equal(got_mode, mode) and np.array_equal(got_cost, cost)
    leaf = leaf.cpu().numpy().astype(bool)
    assert np.array_equal(leaf, ref["leaf"].astype(bool)) and np.array_equal(ctu_cost.cpu().numpy(), ref["ctu_cost"])
    assert np.array_equal(ctu_leaves.cpu().numpy(), ref["ctu_leaves"])
    leaves = np.nonzero(leaf[0])[0]
    ang = _is_angular(mode[0, leaves])
    odd = (mode[0, leaves][ang].astype(int) - BASE) % 2 == 1
    assert ang.any() and (~ang).any() and odd.any()           # angular leaves, refined ones among them, and others
    assert int(sk.item()) - (nct * mipgpu.PART_MAX_LEAVES - leaves.size) == 0     # no leaf is skipped
    got = _host(canvas)
    assert np.all(got[w * h:] == FILL)
    want = _leaf_blocks(frame, w, h, mode[0], leaves)         # angular leaves: angular_ref.predict
    expect = np.full((h, w), FILL, np.uint16)
    _, x, y, bw, bh = layout.cu_geometry(w, h, leaves)
    for i, cu in enumerate(leaves):
        expect[y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] = want[int(cu)]
    bad = np.argwhere(got[:w * h].reshape(h, w) != expect)
    assert bad.size == 0, (len(bad), bad[:4])
    cols = layout.ctu_grid(w, h)[0]
    for ctu in np.nonzero(ref["ctu_cost"][0] != UN)[0]:       # no PRED_NONE sample inside a partitioned CTU
        cy, cx = 128 * (ctu // cols), 128 * (ctu % cols)
        assert not np.any(got[:w * h].reshape(h, w)[cy:cy + 128, cx:cx + 128] == FILL), ctu
