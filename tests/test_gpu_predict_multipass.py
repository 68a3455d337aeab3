"""The prediction kernel on lists longer than one round of its grid, and the host prediction on
more frames than the engine's buffers hold.

predict_kernel is grid-stride: at most 4096 workgroups of 4 waves, 4 list items per wave and pass
(tests/launch_caps.py), so one round is 65 536 items and a wave's consecutive passes are the quads
q and q + 16 384.  Every pass reuses the wave's LDS words (top, left, red, rpred, anc), laid out for
four 16-lane groups when no item of the quad has more than 64 samples and for the whole wave
otherwise, with wave-level fences only between the passes.  The lists here hold 2 1/3 rounds, so
every wave runs a second pass and some a third, and the CPU tests assert -- for the list alone,
before any launch -- that the path changes (16 lanes <-> whole wave) and the item-kind changes
(MIP <-> Planar / DC, written <-> rejected) between a wave's passes occur in numbers.

 1. a dense packed list drawn from a pool of (frame, cu, mode) triples whose reference blocks
    (tests/predict_ref.py, tests/intra_ref.py) are computed once, 15 % rejected entries;
 2. the partition's own list shape [frames][CTUs][1024], more than half of it padding, on the
    device and through the host call (75 frames on an engine that holds 3);
 3. the host call with an engine filter on 7 frames where the engine holds 6: temporary input and
    reference blocks, the filter launched per max_batch frames.
"""
from functools import lru_cache

import numpy as np
import pytest

import edge_sweep_cases as E
import intra_cases as IC
import intra_ref as I
import launch_caps as L
import mipgpu
import oracle_lib as O
import partition_ref as R
import predict_ref as P
from mipgpu import MipEngine, layout
from test_gpu_multipass import _batch_order
from test_gpu_predict_regular import CHAIN_CASES, FILL, FILTER, MODES, _composition, _dev, _dev_items, _host, _sentinel, regular_blocks

gpu = pytest.mark.gpu
UN = layout.UNAVAILABLE
W, H = 136, 72
ROUND = L.PREDICT_ITEMS_PER_ROUND                            # 65 536 items: one pass of every wave
GUARD = 4096                                                 # sentinel samples behind out_samples
PAD_ITEM = np.array((-1, -1, -1, 0, 0), mipgpu.PRED_ITEM)    # the partition's padding entry
# the eight kinds of rejected entries of test_mixed_list_of_mip_regular_and_rejected_items
KINDS = ("frame", "cu", "unavailable", "mode_ff", "mode_f2", "pitch", "offset", "past_end")
MIP, REGULAR, REJECTED = 0, 1, 2                             # what an entry is to the MIP_PRED_REGULAR instance


# ---------------------------------------------------------------- 1. dense list
@lru_cache(maxsize=None)
def _pool():
    """Distinct (frame, cu, mode) triples on the three frames of intra_cases: per frame a CU sample
    of every shape, each CU with one seeded random MIP mode, Planar and DC, and the reference block
    of each triple (flat uint16), computed once."""
    frames, _, un, _ = IC.case(W, H, None)
    rng = np.random.default_rng(0x9E0)
    frame, cu, mode, blocks, shapes = [], [], [], [], set()
    for f in range(len(frames)):
        cus = P.sample_cus(W, H, un, seed=0x9E1 + f, per_shape=1)
        shape, x, y, _, _ = layout.cu_geometry(W, H, cus)
        shapes |= set(int(s) for s in shape)
        regular = regular_blocks(frames[f], W, H, cus)
        for i, k in enumerate(cus):
            pred = P.CuPredictor(frames[f], x[i], y[i], shape[i])
            m = int(rng.integers(0, layout.SHAPES[shape[i]].total_modes))
            for md, blk in ((m, pred.predict(m)), (I.MODE_PLANAR, regular[int(k)][0]), (I.MODE_DC, regular[int(k)][1])):
                frame.append(f)
                cu.append(int(k))
                mode.append(md)
                blocks.append(np.ascontiguousarray(blk, np.uint16).reshape(-1))
    assert shapes == set(range(layout.NUM_SHAPES))           # all 47 shapes at this size
    frame, cu, mode = np.array(frame), np.array(cu), np.array(mode)
    assert len(set(zip(frame.tolist(), cu.tolist(), mode.tolist()))) == frame.size
    assert max(int(b.max()) for b in blocks) <= 1023 < FILL
    return dict(frame=frame, cu=cu, mode=mode, blocks=blocks, area=np.array([b.size for b in blocks]), un=un)


@lru_cache(maxsize=None)
def _dense_list():
    """The list of 2 1/3 rounds: per entry first the size class (<= 64 samples with probability
    0.8 -- a quad takes the 16-lane path only when all four of its written items are small), then
    a triple of that class; 15 % of the entries are then made one of the eight rejected kinds.
    Values of rejected entries are chosen so that a kernel that did not check them would still
    stay inside the tensors of the test: a spare frame lies before and three behind the call's
    frames, a narrower pitch keeps the block inside its own reserved block, and the guard is as
    long as the largest block."""
    pool = _pool()
    n = L.multipass_work(ROUND)
    rng = np.random.default_rng(0xD15)
    small, large = np.nonzero(pool["area"] <= 64)[0], np.nonzero(pool["area"] > 64)[0]
    pick = np.where(rng.random(n) < 0.8, small[rng.integers(0, small.size, n)], large[rng.integers(0, large.size, n)])
    kind = np.where(rng.random(n) < 0.15, rng.integers(0, len(KINDS), n), -1)
    frame, cu, mode = pool["frame"][pick], pool["cu"][pick].copy(), pool["mode"][pick]
    dead = np.nonzero(pool["un"])[0]
    is_kind = {k: kind == i for i, k in enumerate(KINDS)}
    cu[is_kind["unavailable"]] = dead[rng.integers(0, dead.size, is_kind["unavailable"].sum())]
    items, total = mipgpu.pred_items(W, H, frame, cu, mode, nframes=3)
    reserved = items["offset"].copy()                        # packed: blocks back to back in list order
    _, _, _, bw, bh = layout.cu_geometry(W, H, cu)
    area = (bw * bh).astype(np.int64)
    assert np.array_equal(reserved, np.cumsum(area) - area) and total == area.sum()
    items["frame"][is_kind["frame"]] = -1
    whole_pad = is_kind["frame"] & (np.arange(n) % 2 == 0)   # half of them: the partition's padding entry
    items[whole_pad] = PAD_ITEM
    items["cu"][is_kind["cu"]] = pool["un"].size
    items["mode"][is_kind["mode_ff"]] = 0xFF
    items["mode"][is_kind["mode_f2"]] = 0xF2
    items["pitch"][is_kind["pitch"]] -= 4                    # below the block's width, still a multiple of 4
    items["offset"][is_kind["offset"]] += 2
    items["offset"][is_kind["past_end"]] = total - 4         # starts inside out_samples, ends past it
    assert area.max() <= GUARD and all(v.sum() >= 1000 for v in is_kind.values())
    written = kind < 0
    cls = np.where(written, np.where(np.isin(mode, MODES), REGULAR, MIP), REJECTED)
    return dict(items=items, total=total, pick=pick, kind=kind, cls=cls, reserved=reserved, area=area, large=area > 64)


def _written(d, regular):
    """Entries the kernel instance writes: the MIP-only one rejects Planar / DC entries too."""
    return d["cls"] == MIP if not regular else d["cls"] != REJECTED


def _quads(flags_per_item):
    """Per quad of four consecutive items: any of them has the flag."""
    n = flags_per_item.size
    padded = np.zeros(-(-n // L.PREDICT_ITEMS_PER_WAVE) * L.PREDICT_ITEMS_PER_WAVE, bool)
    padded[:n] = flags_per_item
    return padded.reshape(-1, L.PREDICT_ITEMS_PER_WAVE).any(axis=1)


def test_dense_list_reaches_a_third_pass_and_every_transition():
    """Preconditions of the dense-list GPU test, on the list alone."""
    d = _dense_list()
    n = d["items"].size
    assert n == 152917 and L.passes(n, ROUND) == (2, 3)
    assert d["total"] <= 64 << 20, d["total"]
    print("dense list: %d items, %d packed samples, %d rejected" % (n, d["total"], (d["cls"] == REJECTED).sum()))
    for regular in (True, False):
        on = _written(d, regular)
        wave_path = _quads(on & d["large"])                  # the quad takes the whole-wave path
        before, after = wave_path[:-L.PREDICT_QUADS_PER_ROUND], wave_path[L.PREDICT_QUADS_PER_ROUND:]
        up, down = np.mean(~before & after), np.mean(before & ~after)
        print("regular=%s: 16-lane -> whole-wave %.3f, whole-wave -> 16-lane %.3f of %d pass pairs" % (regular, up, down, before.size))
        assert up >= 0.10 and down >= 0.10, (regular, up, down)
        # a 16-lane group's item in consecutive passes (65 536 is a multiple of 4: the same group),
        # all of them and those whose quads take the 16-lane path in both passes
        cls = np.where(on, d["cls"], REJECTED)
        a, b = cls[:-ROUND], cls[ROUND:]
        item_wave_path = np.repeat(wave_path, L.PREDICT_ITEMS_PER_WAVE)[:n]
        both_small = ~item_wave_path[:-ROUND] & ~item_wave_path[ROUND:]
        wanted = [(REJECTED, MIP), (MIP, REJECTED)]
        if regular:
            wanted += [(MIP, REGULAR), (REGULAR, MIP), (REJECTED, REGULAR), (REGULAR, REJECTED)]
        for x, y in wanted:
            every, grouped = int(np.sum((a == x) & (b == y))), int(np.sum((a == x) & (b == y) & both_small))
            print("regular=%s: class %d -> %d: %d pairs, %d on the 16-lane path in both passes" % (regular, x, y, every, grouped))
            assert grouped >= 100, (regular, x, y, every, grouped)


def _expected_dense(d, regular):
    """The whole output tensor (out_samples + guard) by scatter per pool entry, and the skipped count."""
    pool = _pool()
    on = _written(d, regular)
    exp = np.full(d["total"] + GUARD, FILL, np.uint16)
    members = np.nonzero(on)[0]
    members = members[np.argsort(d["pick"][members], kind="stable")]
    entries, first = np.unique(d["pick"][members], return_index=True)
    for p, group in zip(entries, np.split(members, first[1:])):
        blk = pool["blocks"][p]
        assert np.all(d["items"]["offset"][group] == d["reserved"][group])
        exp[d["reserved"][group][:, None] + np.arange(blk.size)[None, :]] = blk
    return exp, int((~on).sum())


def _describe(d, samples):
    """Which entries the output samples belong to: (item, pass, class, rejected kind, area, quad is large)."""
    idx = np.searchsorted(d["reserved"], samples, side="right") - 1
    return [(int(i), int(i // ROUND), int(d["cls"][i]), int(d["kind"][i]), int(d["area"][i]), bool(d["large"][i // 4 * 4:i // 4 * 4 + 4].any()))
            for i in np.unique(idx)[:6]]


@gpu
@pytest.mark.parametrize("regular", (True, False), ids=("regular", "mip_only"))
def test_dense_list_of_three_passes(gpu_available, regular):
    """The whole tensor bit for bit, the guard and every rejected entry's reserved block untouched,
    the skipped word exact -- on both kernel instances (the MIP-only one rejects the Planar / DC
    entries, whose blocks then stay as they were)."""
    import torch
    d = _dense_list()
    exp, n_skipped = _expected_dense(d, regular)
    total = d["total"]
    frames = IC.case(W, H, None)[0]
    spare = np.full((1, H, W), 1023, np.uint16)
    d_all = _dev(np.concatenate([spare, frames, spare, spare, spare]))
    out = _sentinel(total + GUARD)
    sk = torch.zeros(1, dtype=torch.int32, device="cuda")
    with MipEngine(W, H) as eng:
        eng.predict_device(d_all[1:1 + len(frames)], _dev_items(d["items"]), out[:total], skipped=sk, regular=regular)
        torch.cuda.synchronize()
    got = _host(out)
    assert np.all(got[total:] == FILL)                       # the guard
    bad = np.nonzero(got[:total] != exp[:total])[0]
    assert bad.size == 0, (bad.size, bad[:4], _describe(d, bad))
    off = ~_written(d, regular)                              # reserved blocks of entries not written
    where = np.repeat(d["reserved"][off], d["area"][off]) + np.arange(d["area"][off].sum()) - np.repeat(np.cumsum(d["area"][off]) - d["area"][off], d["area"][off])
    assert np.all(got[where] == FILL)
    assert int(sk.item()) == n_skipped
    assert n_skipped == (d["cls"] == REJECTED).sum() + (0 if regular else (d["cls"] == REGULAR).sum())


# ---------------------------------------------------------------- 2. the partition's list shape
def _batch_items(ref_items, sel, w, h):
    """The reference's items [P, nCTUs, 1024] of the pool frames `sel`, with the batch index in
    `frame` and `offset`; padding entries stay {-1, -1, -1, 0, 0}.  Returns (items, real)."""
    items = np.array(ref_items[sel], copy=True)
    real = items["frame"] >= 0
    delta = (np.arange(len(sel)) - sel).astype(np.int64)[:, None, None]
    items["frame"] = np.where(real, items["frame"] + delta, items["frame"])
    items["offset"] = np.where(real, items["offset"] + delta * (w * h), items["offset"])
    assert np.all(items["frame"][real] == np.broadcast_to(np.arange(len(sel))[:, None, None], real.shape)[real])
    assert np.all(items[~real] == PAD_ITEM)
    return items, real


@lru_cache(maxsize=None)
def _pool_items(w, h, filt):
    """partition_ref's items of the CPU composition's three frames (frame-layout entries)."""
    frames, want = _composition(w, h, filt)
    ref = R.partition_frames(want["best_cost"], w, h, E.CHAIN_PENALTY, best_mode=want["best_mode"])
    for key in ("leaf", "ctu_cost", "ctu_leaves"):
        assert np.array_equal(ref[key], want[key]), key
    return frames, want, ref["items"]


PARTITION_FRAMES = 75


@lru_cache(maxsize=None)
def _partition_list():
    frames, want, ref_items = _pool_items(W, H, None)
    nct = layout.num_ctus(W, H)
    assert nct == 2 and PARTITION_FRAMES * nct * mipgpu.PART_MAX_LEAVES >= L.multipass_work(ROUND)
    sel = _batch_order(len(frames), PARTITION_FRAMES, nct * mipgpu.PART_MAX_LEAVES, ROUND, 0x75A)
    items, real = _batch_items(ref_items, sel, W, H)
    return frames, want, sel, items.reshape(-1), real.reshape(-1)


def _host_list(items, real):
    """The list for the host call: mip_predict_frames validates `frame` and `cu` on the host and
    refuses the partition's padding entries, so they name frame 0 / cu 0 there and keep mode -1,
    pitch 0, offset 0 -- still entries the kernel rejects and counts, at the same list positions."""
    host = items.copy()
    host["frame"][~real] = 0
    host["cu"][~real] = 0
    return host


def test_partition_list_is_multipass_and_mostly_padding():
    """Preconditions of the two partition-list GPU tests, on the CPU composition alone."""
    frames, want, sel, items, real = _partition_list()
    n = items.size
    assert n == 153600 and L.passes(n, ROUND) == (2, 3)
    leaf_modes = want["best_mode"][want["leaf"].astype(bool)]
    counts = [int((leaf_modes < 32).sum()), int((leaf_modes == I.MODE_PLANAR).sum()), int((leaf_modes == I.MODE_DC).sum())]
    print("partition list: %d entries, %d leaves (%.1f %% padding); pool leaves MIP / Planar / DC: %s" %
          (n, real.sum(), 100 * np.mean(~real), counts))
    assert all(counts) and sum(counts) == leaf_modes.size
    assert np.mean(~real) > 0.5
    assert real.sum() == want["ctu_leaves"][sel].sum()
    assert np.all(want["ctu_cost"] != UN) and not np.any(want["pred"] == mipgpu.PRED_NONE)   # every CTU has a partition
    assert want["pred"].max() < min(FILL, mipgpu.PRED_NONE)
    # a wave's item kinds change between its passes here too
    before, after = real[:-ROUND], real[ROUND:]
    assert np.sum(before & ~after) >= 100 and np.sum(~before & after) >= 100


@gpu
def test_partition_shaped_list_on_the_device(gpu_available):
    """75 frames x 2 CTUs x 1024 entries in one launch into a sentinel canvas: every frame of the
    canvas is the pool frame's CPU prediction, nothing else is written, and skipped counts exactly
    the padding."""
    import torch
    frames, want, sel, items, real = _partition_list()
    n = PARTITION_FRAMES * W * H
    canvas = _sentinel(n + GUARD)
    sk = torch.zeros(1, dtype=torch.int32, device="cuda")
    with MipEngine(W, H) as eng:
        eng.predict_device(_dev(frames[sel]), _dev_items(items), canvas[:n], skipped=sk, regular=True)
        torch.cuda.synchronize()
    got = _host(canvas)
    assert np.all(got[n:] == FILL)
    got = got[:n].reshape(PARTITION_FRAMES, H, W)
    bad = np.argwhere(got != want["pred"][sel])
    assert bad.size == 0, (len(bad), bad[:4], int((got == FILL).sum()))
    assert not np.any(got == FILL)
    assert int(sk.item()) == items.size - int(want["ctu_leaves"][sel].sum()) == int((~real).sum())


@gpu
def test_partition_shaped_list_through_the_host_call(gpu_available):
    """The same list through mip_predict_frames_ex on an engine with the default max_batch: its
    buffers hold 3 frames, the call's 75 go through a temporary input block.  The list as the
    partition writes it is refused (frame -1 is outside the call's frames: the host call's
    contract); with the padding renamed to rejected entries of frame 0 the output is the device's."""
    frames, want, sel, items, real = _partition_list()
    n = PARTITION_FRAMES * W * H
    with MipEngine(W, H) as eng:
        assert eng.max_batch == 1                            # hp_frames = 3 < 75
        with pytest.raises(mipgpu.MipError, match="frame"):
            eng.predict(frames[sel], items, n, regular=True)
        got, skipped = eng.predict(frames[sel], _host_list(items, real), n, regular=True)
    bad = np.argwhere(got.reshape(PARTITION_FRAMES, H, W) != want["pred"][sel])
    assert bad.size == 0, (len(bad), bad[:4], int((got == mipgpu.PRED_NONE).sum()))
    assert skipped == items.size - int(want["ctu_leaves"][sel].sum())


# ---------------------------------------------------------------- 3. engine filter, more frames than the engine holds
FILTERED_FRAMES = 7


@gpu
@pytest.mark.parametrize("w,h", [(136, 64), (72, 64)], ids=("136x64", "72x64"))
def test_host_prediction_filters_more_frames_than_the_engine_holds(gpu_available, w, h):
    """max_batch = 2: the engine's buffers hold 6 frames, the call has 7 -- temporary input and
    reference blocks and four filter launches, the last of one frame.  The engine serves a
    one-frame prediction and a search afterwards."""
    assert (w, h, FILTER) in CHAIN_CASES
    frames, want, ref_items = _pool_items(w, h, FILTER)
    # a seeded order of the three pool frames; the last frame (a filter launch of its own) differs
    # from the first of the call and from the one before it
    sel = np.random.default_rng(0x7F + w).permutation(len(frames))[[0, 1, 2, 1, 0, 2, 1]]
    assert sel.size == FILTERED_FRAMES and np.unique(sel).size == len(frames) and sel[-1] not in (sel[0], sel[-2])
    items, real = _batch_items(ref_items, sel, w, h)
    items = items[real]                                      # (the host call refuses the padding's frame -1)
    one, one_real = _batch_items(ref_items, np.array([1]), w, h)
    has = want["ctu_cost"] != UN
    assert has.any(axis=1).all() and has.all() == ((w, h) != (136, 64))
    assert items.size == want["ctu_leaves"][sel].sum() > 0
    cost = O.engine_search(frames[2], FILTER, 0)
    with MipEngine(w, h, filter=FILTER, max_batch=2) as eng:
        got, skipped = eng.predict(frames[sel], items, FILTERED_FRAMES * w * h, regular=True)
        again, again_skipped = eng.predict(frames[1], one[one_real], w * h, regular=True)
        searched = eng.search(frames[2])
    got = got.reshape(FILTERED_FRAMES, h, w)
    bad = np.argwhere(got != want["pred"][sel])
    assert bad.size == 0, (len(bad), bad[:4])
    assert skipped == 0 and again_skipped == 0
    cols, _ = layout.ctu_grid(w, h)
    for f, c in np.argwhere(~has[sel]):                      # the CTU without a partition
        assert np.all(got[f, 128 * (c // cols):128 * (c // cols) + 128, 128 * (c % cols):128 * (c % cols) + 128] == mipgpu.PRED_NONE)
    assert np.any(~has[sel]) == ((w, h) == (136, 64))
    assert np.array_equal(again.reshape(h, w), want["pred"][1])
    assert np.array_equal(searched["cost"][0], cost)
