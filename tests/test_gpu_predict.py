"""Prediction output on the GPU (mip_predict_device / mip_predict_frames): the emitted blocks
are the restatement's (tests/predict_ref.py, pinned to the oracle by tests/test_predict_cpu.py)
bit for bit, their SAD / SATD are the engine's own table entries, nothing but the blocks is
written, and a bad device list entry is skipped, never an out-of-bounds access."""
from functools import lru_cache

import numpy as np
import pytest

import mipgpu
import oracle_lib as O
import predict_ref as P
from mipgpu import MipEngine, layout
from mipgpu.synth import synth_frame, synth_frames

pytestmark = pytest.mark.gpu

FILTER = "filterFrame_1d_int"
FILL = 0xABCD
PREFIX = np.cumsum([0] + [s.ncu for s in layout.SHAPES])


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def _dev_items(items):
    return _dev(items.view(np.uint8))


def _host(t):
    return t.cpu().numpy().view(np.uint16)


@lru_cache(maxsize=None)
def _case_136():
    """136x72, separable 3-tap filter: frame, references, the sampled CUs."""
    w, h = 136, 72
    frame = synth_frame(w, h, 0x51, 1)
    refs = O.filter_frame(frame, FILTER, 0)
    cus = P.sample_cus(w, h, mipgpu.unavailable_cus(w, h, FILTER))
    return w, h, frame, refs, cus


@lru_cache(maxsize=None)
def _predictor(cu):
    w, h, _, refs, _ = _case_136()
    shape, x, y, _, _ = layout.cu_geometry(w, h, [cu])
    return P.CuPredictor(refs, x[0], y[0], shape[0])


def _all_modes(w, h, cus):
    shape = layout.cu_geometry(w, h, cus)[0]
    nm = np.array([layout.SHAPES[s].total_modes for s in shape])
    return np.repeat(cus, nm), np.concatenate([np.arange(n) for n in nm])


def _check_packed(w, h, refs, items, got, skip=()):
    shape, x, y, bw, bh = layout.cu_geometry(w, h, items["cu"])
    cache = {}
    for i, it in enumerate(items):
        if i in skip:
            continue
        key = int(it["cu"])
        if key not in cache:
            cache[key] = P.CuPredictor(refs, x[i], y[i], shape[i])
        want = cache[key].predict(it["mode"])
        blk = got[it["offset"]:it["offset"] + bw[i] * bh[i]].reshape(bh[i], bw[i])
        assert np.array_equal(blk, want), (i, int(it["cu"]), int(it["mode"]), layout.SHAPES[shape[i]].name)


def test_exact_samples_packed_engine_filter(gpu_available):
    import torch
    w, h, frame, refs, cus = _case_136()
    _, x, y, _, _ = layout.cu_geometry(w, h, cus)
    # the 512 padding and the F[x-1] / F[(y-1)*W] corner rules
    assert ((x == 0) & (y == 0)).any() and ((x == 0) & (y > 0)).any() and ((y == 0) & (x > 0)).any()
    cu, mode = _all_modes(w, h, cus)
    items, total = mipgpu.pred_items(w, h, 0, cu, mode)
    with MipEngine(w, h, filter=FILTER) as eng:
        got, skipped = eng.predict(frame, items, total)
        assert skipped == 0
        out = torch.full((total,), FILL - 65536, dtype=torch.int16, device="cuda")
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.predict_device(_dev(frame[None]), _dev_items(items), out, skipped=sk)
        torch.cuda.synchronize()
        assert int(sk.item()) == 0
    _check_packed(w, h, refs, items, got)
    assert np.array_equal(_host(out), got)
    assert refs.max() > 1023 and got.max() <= 1023 + 1023  # (boundary samples enter the interpolation)


def test_exact_samples_packed_caller_refs(gpu_available):
    import torch
    w, h = 256, 136
    frame, refs = synth_frame(w, h, 0x99, 1), synth_frame(w, h, 0x9A, 1)
    cus = P.sample_cus(w, h, mipgpu.unavailable_cus(w, h), seed=0x9A, per_shape=2)
    _, x, y, _, _ = layout.cu_geometry(w, h, cus)
    assert ((x == 0) & (y == 0)).any() and ((x == 0) & (y > 0)).any() and ((y == 0) & (x > 0)).any()
    cu, mode = _all_modes(w, h, cus)
    items, total = mipgpu.pred_items(w, h, 0, cu, mode)
    with MipEngine(w, h) as eng:
        got, skipped = eng.predict(frame, items, total, refs=refs)
        assert skipped == 0
        out = torch.full((total,), FILL - 65536, dtype=torch.int16, device="cuda")
        eng.predict_device(_dev(frame[None]), _dev_items(items), out, refs=_dev(refs[None]))
        torch.cuda.synchronize()
    _check_packed(w, h, refs, items, got)
    assert np.array_equal(_host(out), got)


@pytest.mark.parametrize("filt", [None, "filterFrame_2d_float_5x5_quarterCtu"])
def test_blocks_reproduce_the_engines_tables(gpu_available, filt):
    """SAD, SATD and min(2 SAD, SATD) recomputed from the GPU's blocks are the entries of the
    engine's own tables (pinned to the reference's kernels by the golden fixtures)."""
    w, h = 264, 136
    frame = synth_frame(w, h, 0x77, 0)
    nct = layout.num_ctus(w, h)
    un = mipgpu.unavailable_cus(w, h, filt).reshape(nct, layout.CUS_PER_CTU)
    names = ["ALL_AL_4x4", "ALL_AL_8x8", "ALL_AL_16x16", "ALL_AL_64x64", "ALL_AL_32x4", "ALL_NA_16x32"]
    assert [layout.SHAPE_BY_NAME[n].size_id for n in names] == [0, 1, 2, 2, 1, 2]
    lists = []
    for n in names:
        s = layout.SHAPE_BY_NAME[n]
        ctu, c = np.nonzero(~un[:, PREFIX[s.index]:PREFIX[s.index + 1]])
        assert c.size
        lists.append((s, ctu, c))
    cu = np.concatenate([np.repeat(ctu * layout.CUS_PER_CTU + PREFIX[s.index] + c, s.total_modes) for s, ctu, c in lists])
    mode = np.concatenate([np.tile(np.arange(s.total_modes), c.size) for s, ctu, c in lists])
    items, total = mipgpu.pred_items(w, h, 0, cu, mode)
    with MipEngine(w, h, filter=filt, want_sad_satd=True) as eng:
        tab = eng.search(frame, sad_satd=True)
        got, skipped = eng.predict(frame, items, total)
    assert skipped == 0
    pos = 0
    for s, ctu, c in lists:
        m, n = s.total_modes, c.size
        blocks = got[pos:pos + n * m * s.w * s.h].reshape(n, m, s.h, s.w)
        pos += blocks.size
        _, x, y, _, _ = layout.cu_geometry(w, h, ctu * layout.CUS_PER_CTU + PREFIX[s.index] + c)
        idx = (y[:, None, None] + np.arange(s.h)[None, :, None]).astype(np.int64) * w + x[:, None, None] + np.arange(s.w)[None, None, :]
        orig = frame.reshape(-1)[idx][:, None]               # [n, 1, h, w], linear indexes
        entry = (ctu * layout.COSTS_PER_CTU + s.cost_offset + c * m)[:, None] + np.arange(m)[None, :]
        sad, satd = P.sad_blocks(orig, blocks), P.satd_blocks(orig, blocks)
        assert np.array_equal(sad, tab["sad"][0][entry]), s.name
        assert np.array_equal(satd, tab["satd"][0][entry]), s.name
        assert np.array_equal(np.minimum(2 * sad, satd), tab["cost"][0][entry]), s.name
    assert pos == total


def test_frame_layout_writes_the_blocks_and_nothing_else(gpu_available):
    import torch
    w, h, frame, refs, _ = _case_136()
    s = layout.SHAPE_BY_NAME["ALL_AL_16x16"]
    nct = layout.num_ctus(w, h)
    cu = (np.arange(nct)[:, None] * layout.CUS_PER_CTU + PREFIX[s.index] + np.arange(s.ncu)[None, :]).reshape(-1)
    un = mipgpu.unavailable_cus(w, h, FILTER)[cu]
    _, x, y, _, _ = layout.cu_geometry(w, h, cu)
    assert un.any() and ((x + s.w > w) & ~un).any()          # below the frame; wrapped right of it
    guard = 4096
    with MipEngine(w, h, filter=FILTER) as eng:
        best = eng.search(frame, best=True)["best_mode"][0][cu]
        assert np.array_equal(best == 0xFF, un)
        items, total = mipgpu.pred_items(w, h, 0, cu, best, layout="frame", nframes=1)
        assert total == w * h
        buf = torch.full((total + guard,), FILL - 65536, dtype=torch.int16, device="cuda")
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.predict_device(_dev(frame[None]), _dev_items(items), buf[:total], skipped=sk)
        torch.cuda.synchronize()
        host, host_skipped = eng.predict(frame, items, total)
    got = _host(buf)
    # the restatement scattered at linear indexes; wrapped CUs overlap their left neighbours'
    # next row, where either block may win (mipgpu.h)
    count = np.zeros(total, np.int64)
    cand = np.zeros((2, total), np.uint16)
    for i in np.nonzero(~un)[0]:
        blk = _predictor(int(cu[i])).predict(best[i])
        idx = ((y[i] + np.arange(s.h))[:, None] * w + x[i] + np.arange(s.w)[None, :]).reshape(-1)
        assert count[idx].max() < 2
        cand[count[idx], idx] = blk.reshape(-1)
        count[idx] += 1
    assert (count == 0).any() and (count == 2).any()
    for name, res, empty in (("device", got[:total], FILL), ("host", host, mipgpu.PRED_NONE)):
        assert np.all(res[count == 0] == empty), name
        one, two = count == 1, count == 2
        assert np.array_equal(res[one], cand[0][one]), name
        assert np.all((res[two] == cand[0][two]) | (res[two] == cand[1][two])), name
    assert np.all(got[total:] == FILL)                        # the guard behind the canvas
    assert int(sk.item()) == un.sum() == host_skipped


def test_bad_device_list_entries_are_skipped(gpu_available):
    """Every bad entry sits next to a good one; the values are chosen so that even an
    unchecked entry would stay inside the tensors allocated here (a spare frame, an output
    tensor of twice out_samples)."""
    import torch
    w, h = 136, 72
    frames = synth_frames(w, h, 2, 0xBAD, 1)                  # frame 1 is the spare
    nct = layout.num_ctus(w, h)
    c16 = PREFIX[layout.SHAPE_BY_NAME["ALL_AL_16x16"].index] + 9
    c4 = PREFIX[layout.SHAPE_BY_NAME["ALL_AL_4x4"].index] + 40
    c64 = 0
    cu = np.array([c16, c16, c4, c4, c64, c16, c16, c4, c4, c16, c4, c16, c4, c4])
    mode = np.array([3, 3, 17, 17, 5, 2, 2, 9, 9, 7, 30, 1, 4, 4])
    items, total = mipgpu.pred_items(w, h, 0, cu, mode)
    bad = {1: "frame == nframes", 3: "cu == nctus*5380", 6: "pitch < w", 8: "misaligned offset",
           10: "offset == out_samples", 12: "block straddles the end", 13: "negative mode"}
    items["frame"][1] = 1
    items["cu"][3] = nct * layout.CUS_PER_CTU
    items["pitch"][6] = 8
    items["offset"][8] += 2
    items["offset"][10] = total
    items["offset"][12] = total - 4
    items["mode"][13] = -1
    out = torch.full((2 * total,), FILL - 65536, dtype=torch.int16, device="cuda")
    sk = torch.zeros(1, dtype=torch.int32, device="cuda")
    with MipEngine(w, h) as eng:
        eng.predict_device(_dev(frames)[:1], _dev_items(items), out[:total], skipped=sk)
        torch.cuda.synchronize()
    got = _host(out)
    assert int(sk.item()) == len(bad)
    good = items.copy()
    good["cu"][3] = c4                                        # (geometry of the reserved blocks)
    _check_packed(w, h, frames[0], good, got, skip=set(bad))
    written = np.zeros(2 * total, bool)
    _, _, _, bw, bh = layout.cu_geometry(w, h, good["cu"])
    for i, it in enumerate(good):
        if i not in bad:
            written[it["offset"]:it["offset"] + bw[i] * bh[i]] = True
    # the reserved blocks of the bad entries, the tail and the second half are untouched
    assert np.all(got[~written] == FILL)


def test_batch_on_a_side_stream_equals_per_frame_host_calls(gpu_available):
    import torch
    w, h, nf = 384, 256, 3
    frames = synth_frames(w, h, nf, 0x5EED, 0)
    rng = np.random.default_rng(5)
    un = mipgpu.unavailable_cus(w, h)
    cus = P.sample_cus(w, h, un, seed=3, per_shape=1)
    shape = layout.cu_geometry(w, h, cus)[0]
    frame = rng.integers(0, nf, cus.size)
    mode = np.array([rng.integers(0, layout.SHAPES[s].total_modes) for s in shape])
    items, total = mipgpu.pred_items(w, h, frame, cus, mode, nframes=nf)
    with MipEngine(w, h, max_batch=nf) as eng:
        stream = torch.cuda.Stream()
        d_frames, d_items = _dev(frames), _dev_items(items)
        out = torch.full((total,), FILL - 65536, dtype=torch.int16, device="cuda")
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            eng.predict_device(d_frames, d_items, out, skipped=sk, stream=stream)
        stream.synchronize()
        got = _host(out)
        assert int(sk.item()) == 0 and not (got == FILL).any()
        sizes = np.diff(np.append(items["offset"], total))
        for f in range(nf):
            sel = np.nonzero(frame == f)[0]
            assert sel.size
            it_f, tot_f = mipgpu.pred_items(w, h, 0, cus[sel], mode[sel])
            want, skipped = eng.predict(frames[f], it_f, tot_f)
            assert skipped == 0
            for j, i in enumerate(sel):
                a = got[items["offset"][i]:items["offset"][i] + sizes[i]]
                assert np.array_equal(a, want[it_f["offset"][j]:it_f["offset"][j] + sizes[i]]), (f, int(cus[i]))
