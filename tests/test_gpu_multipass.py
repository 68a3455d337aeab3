"""The two grid-stride kernels on launches larger than their grid caps: partition_kernel and
intra_kernel take work blockIdx.x, + gridDim.x, ... and reuse their LDS arrays (s_cost,
s_choice and the s_leaf / s_scan overlay; s_org, s_ref, s_left, s_part) for every pass.  Each
batch here holds 2 1/3 rounds of the capped grid (tests/launch_caps.py), so every workgroup
runs a second pass on LDS its first pass wrote and some run a third.  The batch repeats a
small pool of distinct frames in a seeded random order: the expected output is the pool's
reference (tests/partition_ref.py, tests/intra_ref.py) indexed by that order, bit for bit.

The CPU test pins the cap factors to the launchers' text, so the GPU tests cannot fall back to
single-pass coverage when a cap changes."""
import re

import numpy as np
import pytest

import intra_cases as IC
import intra_ref as I
import launch_caps as L
import mipgpu
import partition_cases as C
import partition_ref as R
from mipgpu import MipEngine, layout

gpu = pytest.mark.gpu
UN = layout.UNAVAILABLE


def test_launch_caps_are_the_launchers():
    """Each launcher caps its grid at the helper's factor times the CU count, read from
    hipDeviceAttributeMultiprocessorCount.  Someone who changes a cap changes launch_caps.py with
    it: the GPU tests below size their batches from it."""
    for source, launcher, factor in L.LAUNCHERS:
        body = L.launcher_body(source, launcher)
        found = L.CAP_EXPRESSION.findall(body)
        assert len(found) == 1, (source, found)
        assert found[0] == (str(factor), str(factor)), (source, found)
        assert "hipDeviceAttributeMultiprocessorCount" in body, source
    # the intra kernel's items per CTU, which the alternation argument of the intra test rests on:
    # the shared walk's, which launch_intra and intra_kernel go through
    text = L.window_text()
    assert text.count("constexpr int kItemsPerCtu = 4 + kIntraBlocks;") == 1 and text.count("const bool big = k < 4;") == 1
    assert L.uses_window_rules("mip_intra.hip", "launch_intra", "intra_kernel")
    with open(L.CSRC + "/intra_plan.h") as f:
        assert "constexpr int kIntraBlocks = 16;" in f.read()
    assert L.INTRA_ITEMS_PER_CTU == 4 + 16 and L.INTRA_BIG_ITEMS == 4
    assert L.passes(L.multipass_work(2048), 2048) == (2, 3) and L.passes(18, 2048) == (1, 1)


def test_predict_and_copy_caps_are_the_launchers():
    """The same contract for the prediction kernel (tests/test_gpu_predict_multipass.py) and the
    copy kernel (tests/test_gpu_copy.py): their caps, the items a wave takes per pass and the reach
    of the copy's main loop are the helper's constants, read from the launchers' and kernels' text."""
    with open(L.CSRC + "/mip_predict.hip") as f:
        text = f.read()
    assert "constexpr int kPredWaves = %d;" % L.PREDICT_WAVES in text
    assert "constexpr int kPredItemsPerWave = %d;" % L.PREDICT_ITEMS_PER_WAVE in text
    body = L.launcher_body("mip_predict.hip", "launch_predict")
    assert "per_group = (long long)kPredWaves * kPredItemsPerWave;" in body
    found = re.findall(r"groups\s*=\s*std::min<long long>\(\(a\.n \+ per_group - 1\) / per_group,\s*(\d+)\s*\*\s*(\d+)\);", body)
    assert len(found) == 1 and int(found[0][0]) * int(found[0][1]) == L.PREDICT_GROUPS_CAP == 4096, found
    assert body.count("dim3((unsigned)groups), dim3(64 * kPredWaves)") == 2      # both instances, one grid
    kernel = L.kernel_body("mip_predict.hip", "predict_kernel")
    assert "q = (long long)blockIdx.x * kPredWaves + wv; q < quads; q += (long long)gridDim.x * kPredWaves" in kernel
    assert "idx = q * kPredItemsPerWave + grp;" in kernel and "grp = lane >> 4" in kernel
    assert L.PREDICT_ITEMS_PER_ROUND == L.PREDICT_GROUPS_CAP * L.PREDICT_WAVES * L.PREDICT_ITEMS_PER_WAVE == 65536
    assert L.PREDICT_QUADS_PER_ROUND * L.PREDICT_ITEMS_PER_WAVE == L.PREDICT_ITEMS_PER_ROUND
    assert L.multipass_work(L.PREDICT_ITEMS_PER_ROUND) == 152917
    assert L.passes(152917, L.PREDICT_ITEMS_PER_ROUND) == (2, 3)

    body = L.launcher_body("mip_filter.hip", "launch_copy")
    found = re.findall(r"blocks\s*=\s*std::min<size_t>\(\(size_t\)cus \* (\d+), \(n16 \+ (\d+)\) / (\d+)\);", body)
    assert found == [(str(L.COPY_GROUPS_PER_CU), str(L.COPY_WORDS_PER_GROUP - 1), str(L.COPY_WORDS_PER_GROUP))], found
    assert "hipDeviceAttributeMultiprocessorCount" in body and "dim3(256)" in body
    assert "bytes % 16 || ((uintptr_t)src | (uintptr_t)dst) % 16" in body       # the refusals of test_gpu_copy.py
    kernel = L.kernel_body("mip_filter.hip", "copy_kernel")
    assert "stride = (size_t)gridDim.x * %d;" % L.COPY_WORDS_PER_GROUP in kernel
    assert "i = (size_t)blockIdx.x * %d + threadIdx.x;" % L.COPY_WORDS_PER_GROUP in kernel
    assert "for (; i + %d < n16; i += stride)" % L.COPY_MAIN_LOOP_REACH in kernel
    assert "for (; i < n16; i += 256)" in kernel
    assert L.COPY_MAIN_LOOP_REACH == L.COPY_WORDS_PER_GROUP - 256
    assert L.copy_cap(256) == 2048


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _batch_order(pool, nframes, unit, cap, seed):
    """sel [nframes]: pool frame of every batch frame, seeded random.  `unit` work items per
    frame, `cap` workgroups: asserts that the batch is a multi-pass one and that the content a
    workgroup sees changes from one pass to the next (no period of the grid)."""
    work = nframes * unit
    assert work >= L.multipass_work(cap)
    assert L.passes(work, cap) == (2, 3)                      # every workgroup twice, some three times
    sel = np.random.default_rng(seed).integers(0, pool, nframes)
    assert np.unique(sel).size == pool
    per_item = np.repeat(sel, unit)
    assert np.mean(per_item[:-cap] != per_item[cap:]) > 0.5   # pass p and pass p + 1 of one workgroup
    return sel


# ---------------------------------------------------------------- partition
# (width, height, the two CTUs without a partition and the CTU-relative sample whose covering
# CUs are dead).  264x136: 3x2 CTUs, partial right and below; (20, 36) is partition_cases.impossible's
# sample.  132x132: the right column and the bottom row hold only their first 4 samples.
PARTITION_SIZES = [(264, 136, ((0, 20, 36), (1, 20, 36))), (132, 132, ((0, 20, 36), (3, 0, 0)))]


def _impossible(w, h, ctu, x0, y0):
    if (x0, y0) == (20, 36):
        return C.impossible(w, h, ctu)
    c, m = (a.copy() for a in C.costs(w, h, "holes", 1, seed=11))
    kill = C.covering(w, h, ctu, x0, y0)
    c[:, kill], m[:, kill] = UN, 0xFF
    return c, m


def _partition_pool(w, h, dead):
    """(best_cost, best_mode) [P, ncu] of P = 8 distinct frames: random, ties and holes, two of them
    with a CTU that has no partition (different CTUs), and the reference's outputs for them."""
    parts = [C.costs(w, h, "random", 2), C.costs(w, h, "ties", 2), C.costs(w, h, "holes", 2)]
    parts += [_impossible(w, h, *d) for d in dead]
    cost, mode = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    ref = R.partition_frames(cost, w, h, C.MID_PENALTY, best_mode=mode)
    for k, (ctu, _, _) in enumerate(dead):
        none = ref["ctu_cost"][6 + k] == UN
        assert none[ctu] and none.sum() == 1, (k, ctu)       # exactly that CTU has no partition
    assert len({c.tobytes() for c in cost}) == len(cost) and len({l.tobytes() for l in ref["leaf"]}) >= 6
    return cost, mode, ref


@gpu
@pytest.mark.parametrize("case", PARTITION_SIZES, ids=lambda c: "%dx%d" % c[:2])
def test_partition_multipass(gpu_available, case):
    """2 1/3 rounds of 8 * CUs (frame, CTU) pairs, all four outputs in the guard arena, mid
    penalty: every output whole against the pool reference in batch order."""
    from test_gpu_partition import OUTPUTS, PAD_ITEM, Arena, _dev
    w, h, dead = case
    nct = layout.num_ctus(w, h)
    assert nct >= 2 and (w % 128 or h % 128) and (w, h) in C.SIZES
    cap = L.partition_cap(_cus())
    nframes = -(-L.multipass_work(cap) // nct)
    cost, mode, ref = _partition_pool(w, h, dead)
    sel = _batch_order(len(cost), nframes, nct, cap, 0x9A7 + w)
    arena = Arena(nframes, nct)
    mipgpu.partition_device(_dev(cost[sel]), w, h, penalty=C.MID_PENALTY, best_mode=_dev(mode[sel]),
                            **{k: arena.tensor(k) for k in OUTPUTS})
    got, clean = arena.read(OUTPUTS)
    assert clean
    for key in ("leaf", "ctu_cost", "ctu_leaves"):
        bad = np.argwhere(got[key] != ref[key][sel])
        assert bad.size == 0, (key, len(bad), bad[:4])
    # the reference's items with the batch's frame index in `frame` and `offset`
    want = ref["items"][sel]
    real = want["frame"] >= 0
    delta = (np.arange(nframes) - sel).astype(np.int64)[:, None, None]
    want["frame"] = np.where(real, want["frame"] + delta, want["frame"])
    want["offset"] = np.where(real, want["offset"] + delta * (w * h), want["offset"])
    assert np.all(want["frame"][real] == np.broadcast_to(np.arange(nframes)[:, None, None], real.shape)[real])
    bad = np.argwhere(got["items"] != want)
    assert bad.size == 0, ("items", len(bad), bad[:4])
    assert np.all(got["items"][~real] == PAD_ITEM) and (~real).any()
    # legality on the first and the last frames (first, second and third passes) and the pool's first uses
    sample = sorted(set(range(4)) | set(range(nframes - 4, nframes)) | {int(np.argmax(sel == p)) for p in range(len(cost))})
    C.check_legal(got["leaf"][sample], got["ctu_cost"][sample], got["ctu_leaves"][sample], w, h)


# ---------------------------------------------------------------- intra
def _synthetic_decisions(cost, un, seed):
    """MIP decisions for the merge as tests/test_intra_plan.py makes them: costs around the
    Planar / DC costs, half of them exact ties with the cheaper of the two, 5 % dead CUs."""
    rng = np.random.default_rng(seed)
    avail_cost = np.where(cost == UN, 0, cost).min(axis=2)
    best_cost = (avail_cost + rng.integers(-40, 41, avail_cost.shape) * rng.integers(0, 2, avail_cost.shape)).clip(0).astype(np.int32)
    best_mode = rng.integers(0, 12, best_cost.shape).astype(np.uint8)
    dead = np.broadcast_to(un, best_cost.shape) | (rng.random(best_cost.shape) < 0.05)
    best_cost[dead], best_mode[dead] = UN, 0xFF
    return best_mode, best_cost, dead


@gpu
@pytest.mark.parametrize("filt", (None, IC.FILTER), ids=("orig", "1d_int"))
def test_intra_multipass(gpu_available, filt):
    """2 1/3 rounds of 32 * CUs items at 136x72 (2 CTUs, 40 items per frame), the three tables and
    the merge in one launch.  A workgroup's item index inside the CTU moves by cap % 20 per pass,
    so workgroups go from a 64x64 item (65 s_left rows, 2 s_ref rows) to a 32x32 one (33 rows each)
    and back: stale rows of the other kind would show."""
    from test_gpu_intra import Arena, _dev
    w, h = 136, 72
    frames, _, un, ref = IC.case(w, h, filt)
    nct = layout.num_ctus(w, h)
    unit = nct * L.INTRA_ITEMS_PER_CTU
    cap = L.intra_cap(_cus())
    nframes = -(-L.multipass_work(cap) // unit)
    sel = _batch_order(len(frames), nframes, unit, cap, 0x1A7 + (filt is not None))
    # the kind of item a workgroup has in passes 0 and 1: both changes occur
    k0, k1 = np.arange(cap) % L.INTRA_ITEMS_PER_CTU, (np.arange(cap) + cap) % L.INTRA_ITEMS_PER_CTU
    big0, big1 = k0 < L.INTRA_BIG_ITEMS, k1 < L.INTRA_BIG_ITEMS
    assert cap % L.INTRA_ITEMS_PER_CTU and (big0 & ~big1).any() and (~big0 & big1).any()
    bias = (7, 3)
    cost = ref["cost"][sel]
    best_mode, best_cost, dead = _synthetic_decisions(cost, un, w + nframes)
    with MipEngine(w, h, filter=filt, max_batch=nframes) as eng:
        arena = Arena(nframes, eng.cus_per_frame)
        m, c = _dev(best_mode), _dev(best_cost)
        eng.intra_device(_dev(frames[sel]), bias=bias, best_mode=m, best_cost=c, **{k: arena.tensor(k) for k in IC.TABLES})
        got, clean = arena.read(IC.TABLES)
        got_mode, got_cost = m.cpu().numpy(), c.cpu().numpy()
    assert clean
    for key in IC.TABLES:
        bad = np.argwhere(got[key] != ref[key][sel])
        assert bad.size == 0, (key, len(bad), bad[:4])
    want_mode, want_cost = I.merge(best_mode, best_cost, cost, bias)
    assert np.array_equal(got_mode, want_mode) and np.array_equal(got_cost, want_cost)
    assert (want_mode == I.MODE_PLANAR).any() and (want_mode == I.MODE_DC).any() and (want_mode < 12).any()
    assert np.array_equal(want_mode[dead], best_mode[dead])   # unavailable CUs stay as they are
