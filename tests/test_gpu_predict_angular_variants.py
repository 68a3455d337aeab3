"""Angular block output under the three other settings of (mip_angular_refs, mip_angular_interp) --
ext2: extended lines, 2-tap (angular_ext_predict_kernel); sub4: substituted lines, 4-tap
(angular_tap4_predict_kernel without a length table); ext4: extended lines, 4-tap (the same kernel
with the table) -- on the lists of the default setting's suite (tests/test_gpu_predict_angular.py),
drawn from tests/predict_angular_variant_cases.py: every shape and every mode, also on the 0 / 1023
frame where the cubic overshoots; an engine filter, caller references and the engine's own tables
with the length set that goes with each; mixed quads under the flag matrix with an exact skipped
count; the 8-byte store path; a 2 1/3-round multi-pass scan; and the 4-tap block output at the
frame-edge residues.  Every comparison is bit for bit against the numpy restatements
(tests/angular_ext_ref.py, tests/angular_tap4_ref.py) and leaves nothing out.
tests/test_predict_angular_variants_cpu.py shows on the restatements alone that these lists tell
the four kernels, the two length tables and the clips apart."""
import ctypes

import numpy as np
import pytest

import edge_sweep_cases as E
import mipgpu
import predict_angular_variant_cases as V
import predict_ref as P
from mipgpu import MipEngine, layout
from predict_angular_variant_cases import ALL_CODES, BASE, FILL

pytestmark = pytest.mark.gpu

VARIANT = pytest.mark.parametrize("variant", V.IDS)
TAP4_VARIANT = pytest.mark.parametrize("variant", ("sub4", "ext4"))


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


def _zero():
    import torch
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _engine(w, h, variant, **kw):
    return V.set_variant(MipEngine(w, h, **kw), variant)


def _predict_ex(eng, d_frames, d_items, n, out, out_samples, sk, flags):
    """mip_predict_device_ex with an explicit flags word; returns the status."""
    import torch
    s = torch.cuda.current_stream()
    return mipgpu.library().mip_predict_device_ex(eng._h, d_frames.data_ptr(), None, 1, d_items.data_ptr(), n, out.data_ptr(), out_samples,
                                                  sk.data_ptr(), flags, ctypes.c_void_p(s.cuda_stream))


def _same_packed(got, want, items, note):
    """got == want, sample for sample; on a difference names the first items that hold one."""
    bad = np.nonzero(got != want)[0]
    if bad.size:
        at = np.unique(np.searchsorted(items["offset"], bad, side="right") - 1)[:4]
        raise AssertionError((note, int(bad.size), [(int(items["cu"][i]), int(items["mode"][i]) - BASE) for i in at], got[bad[:4]], want[bad[:4]]))


# ---------------------------------------------------------------- 1. every shape, every mode
@VARIANT
def test_every_shape_every_mode(gpu_available, variant):
    """264x136, frame 1 of tests/intra_cases.py: the CU sample of the default setting's test plus
    CUs of every shape with no, a partial and the full extension on either line, all 65 modes,
    packed; skipped ends at 0 and the samples behind `out` stay.  The 4-tap variants run the same
    list on the 0 / 1023 frame too, where the cubic taps leave the 10-bit range on both sides."""
    import torch
    w, h = V.SIZE
    cus = V.variant_shape_cus()
    items, total = mipgpu.pred_items(w, h, 0, np.repeat(cus, 65), np.tile(ALL_CODES, cus.size))
    d_items = _dev_items(items)
    with _engine(w, h, variant) as eng:
        for which in (0,) if variant == "ext2" else (0, 1):
            want = V.shape_expected(variant, which)
            assert want.size == total
            out, sk = _sentinel(total + 64), _zero()
            eng.predict_device(_dev(V.shape_frames()[which][None]), d_items, out[:total], skipped=sk, angular=True)
            torch.cuda.synchronize()
            got = _host(out)
            assert int(sk.item()) == 0 and np.all(got[total:] == FILL), which
            _same_packed(got[:total], want, items, (variant, which))


# ---------------------------------------------------------------- 2. filter, caller references, the engine's tables
@VARIANT
@pytest.mark.parametrize("source", tuple(V.TABLE_SOURCES))
def test_blocks_and_tables_with_a_filter_and_with_caller_references(gpu_available, source, variant):
    """264x136, the six shapes of the default setting's table test with every CU whose lengths
    differ between the engine's two tables, all 65 modes.  2d_int: the engine's
    filterFrame_2d_int_quarterCtu; 1d_int: filterFrame_1d_int on the 0 / 1023 frame, references up to
    1535; caller_refs: tests/size_sweep.py's on an engine that has a filter of its own.  The blocks
    are the restatement's on those references with the filter's length set (the MIP_FILTER_NONE set
    for the caller's); SAD / SATD / cost recomputed from them are the engine's own angular tables of
    the variant, and those are the restatement's.  Once on the device and once through the host call
    on five frames of an engine with max_batch 2."""
    import torch
    w, h = V.SIZE
    filt, frame, refs, sets, _ = V.table_source(source)
    caller = sets is None
    if source == "1d_int":
        assert E.max_boundary_or_corner(refs, mipgpu.unavailable_cus(w, h, filt), w, h) > 1023
    lists = V.variant_table_lists(source)
    cu = np.concatenate([np.repeat(k, 65) for _, k in lists])
    mode = np.concatenate([np.tile(ALL_CODES, k.size) for _, k in lists])
    items, total = mipgpu.pred_items(w, h, 0, cu, mode)
    spread, five_total = mipgpu.pred_items(w, h, (np.arange(cu.size) * 3) % 5, cu, mode, nframes=5)
    assert five_total == total and np.array_equal(spread["offset"], items["offset"]) and set(spread["frame"]) == set(range(5))
    want = V.table_expected(variant, source)
    ref = V.table_restatement(variant, source)
    with _engine(w, h, variant, filter=filt, max_batch=2) as eng:
        d_frames, d_refs = _dev(frame[None]), _dev(refs[None]) if caller else None
        tab = {k: torch.full((1, eng.cus_per_frame, 65), -7, dtype=torch.int32, device="cuda") for k in ("cost", "sad", "satd")}
        eng.angular_device(d_frames, refs=d_refs, **tab)
        out, sk = _sentinel(total + 64), _zero()
        eng.predict_device(d_frames, _dev_items(items), out[:total], refs=d_refs, skipped=sk, angular=True)
        torch.cuda.synchronize()
        got = _host(out)
        tab = {k: v.cpu().numpy()[0] for k, v in tab.items()}
        five = np.repeat(frame[None], 5, axis=0)
        host, host_skipped = eng.predict(five, spread, total, refs=np.repeat(refs[None], 5, axis=0) if caller else None, angular=True)
    assert int(sk.item()) == 0 and host_skipped == 0 and np.all(got[total:] == FILL)
    _same_packed(got[:total], want, items, (variant, source, "device"))
    _same_packed(host, want, items, (variant, source, "host"))
    for key in ("cost", "sad", "satd"):
        assert np.array_equal(tab[key], ref[key]), (key, variant, source)
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
@VARIANT
def test_mixed_quads_and_the_flag_matrix(gpu_available, variant):
    """The mixed list of the default setting's test over a CU sample that puts four different
    (E_top, E_left) pairs of both classes into one step of a wave's four groups: with flags 4 and 5
    the angular items are the variant's blocks between entries the kernel must leave alone; with 0
    and 1 the output and the skipped count are those of an engine that never touched the switches,
    GPU against GPU, and the restatement's."""
    import torch
    case = V.mixed_variant_case()
    w, h, frame, un, cus, kind, cu, items, total = case
    n, out_samples = items.size, total - 1                    # the last block is one sample too long
    is_ang = np.isin(kind, list(V.ANG_KINDS))
    d_frames, d_items = _dev(np.stack([frame, frame[::-1]])), _dev_items(items)
    lib = mipgpu.library()
    counts = {}
    with _engine(w, h, variant) as eng, MipEngine(w, h) as plain:
        for flags in (0, 1, 4, 5):
            out, sk = _sentinel(2 * total), _zero()
            assert _predict_ex(eng, d_frames, d_items, n, out, out_samples, sk, flags) == 0, lib.mip_last_error()
            torch.cuda.synchronize()
            exp, n_skipped = V.mixed_expected(case, variant, flags)
            got = _host(out)
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, (flags, bad[:4], got[bad[:4]], exp[bad[:4]])
            assert int(sk.item()) == n_skipped, flags
            counts[flags] = n_skipped
            if not flags & mipgpu.PRED_ANGULAR:
                old, sk_old = _sentinel(2 * total), _zero()
                assert _predict_ex(plain, d_frames, d_items, n, old, out_samples, sk_old, flags) == 0, lib.mip_last_error()
                torch.cuda.synchronize()
                assert np.array_equal(_host(old), got) and int(sk_old.item()) == n_skipped, flags
    n_bad = len(V.BAD_KINDS) * V.PER_BAD_KIND + 1
    assert counts[5] == n_bad and counts[1] == n_bad + is_ang.sum() and counts[4] == n_bad + 2 * cus.size
    assert counts[0] == n_bad + is_ang.sum() + 2 * cus.size   # with 4 alone the Planar / DC items are skipped


# ---------------------------------------------------------------- 4. narrow stores and unaligned rows
@VARIANT
@pytest.mark.parametrize("w,h", V.NARROW_SIZES, ids=("132x136", "260x72"))
def test_frame_layout_with_a_pitch_that_is_no_multiple_of_8(gpu_available, w, h, variant):
    """W % 8 == 4: every block takes the 8-byte stores.  The non-overlapping CU set of the default
    setting's test, one launch, modes cycling through all 65; on the device and through the host call."""
    import torch
    frame, cus, shape, x, y, bw, bh, modes, used = V.narrow_case(w, h)
    assert w % 8 == 4 and set(modes) == set(range(2, 67))
    want = V.blocks(variant, frame, w, h, cus)
    items, n_out = mipgpu.pred_items(w, h, 0, cus, BASE + modes, layout="frame", nframes=1)
    assert n_out == w * h and np.all(items["pitch"] % 8 == 4)
    expect = np.full(w * h + 64, FILL, np.uint16)
    canvas = expect[:w * h].reshape(h, w)
    for i, c in enumerate(cus):
        canvas[y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] = want[int(c)][modes[i] - 2]
    with _engine(w, h, variant) as eng:
        out, sk = _sentinel(w * h + 64), _zero()
        eng.predict_device(_dev(frame[None]), _dev_items(items), out[:w * h], skipped=sk, angular=True)
        host, host_skipped = eng.predict(frame, items, n_out, angular=True)
        torch.cuda.synchronize()
        got = _host(out)
    bad = np.argwhere(got[:w * h].reshape(h, w) != canvas)
    assert bad.size == 0 and np.all(got[w * h:] == FILL), (len(bad), bad[:4])
    assert int(sk.item()) == 0 and host_skipped == 0
    assert np.array_equal(host, np.where(expect[:w * h] == FILL, mipgpu.PRED_NONE, expect[:w * h]))


@VARIANT
def test_packed_list_of_4_wide_cus(gpu_available, variant):
    """Packed 4-wide blocks (4x4 to 4x32, pitch 4): 8-byte stores of whole rows, four small blocks
    per wave step and the whole-wave path in one list; on the device and through the host call."""
    import torch
    w, h, frame, cus, bh, modes = V.four_wide_case()
    assert set(bh) == {4, 8, 16, 32}
    want = V.blocks(variant, frame, w, h, cus)
    items, total = mipgpu.pred_items(w, h, 0, cus, BASE + modes)
    assert np.all(items["pitch"] == 4)
    expect = np.concatenate([want[int(c)][m - 2].reshape(-1) for c, m in zip(cus, modes)])
    with _engine(w, h, variant) as eng:
        out, sk = _sentinel(total + 64), _zero()
        eng.predict_device(_dev(frame[None]), _dev_items(items), out[:total], skipped=sk, angular=True)
        host, host_skipped = eng.predict(frame, items, total, angular=True)
        torch.cuda.synchronize()
        got = _host(out)
    assert int(sk.item()) == 0 and host_skipped == 0 and np.all(got[total:] == FILL)
    _same_packed(got[:total], expect, items, (variant, "device"))
    _same_packed(host, expect, items, (variant, "host"))


# ---------------------------------------------------------------- 5. multi-pass
@VARIANT
def test_multipass_scan(gpu_available, variant):
    """The 611 669-entry list of the default setting's test with a CU pool drawn so that, within one
    wave, the item of one pass has its full extension and the item of the next pass, in the same LDS
    words, has none and the same S and M: two rounds and a third of the capped grid, the coefficient words staged once
    before them.  Flags 5, then 4 alone with the Planar items skipped."""
    import torch
    m = V.multipass_variant_list()
    w, h, frame, n, items, total, at, kind = (m[k] for k in ("w", "h", "frame", "n", "items", "total", "at", "kind"))
    expect = V.multipass_expected(m, variant)
    planar = np.zeros(total + 64, bool)
    for i in np.nonzero(kind == 2)[0]:
        c = m["which"][i]
        planar[m["real"]["offset"][i]:m["real"]["offset"][i] + m["bw"][c] * m["bh"][c]] = True
    d_frames, d_items = _dev(frame[None]), _dev_items(items)
    with _engine(w, h, variant) as eng:
        out, sk = _sentinel(total + 64), _zero()
        eng.predict_device(d_frames, d_items, out[:total], skipped=sk, regular=True, angular=True)
        only, sk4 = _sentinel(total + 64), _zero()
        eng.predict_device(d_frames, d_items, only[:total], skipped=sk4, angular=True)
        torch.cuda.synchronize()
        got, got4 = _host(out), _host(only)
    bad = np.nonzero(got != expect)[0]
    assert bad.size == 0, (bad.size, bad[:4], got[bad[:4]], expect[bad[:4]])
    assert int(sk.item()) == n - at.size
    assert planar.any() and np.array_equal(got4, np.where(planar, FILL, expect))
    assert int(sk4.item()) == n - at.size + int((kind == 2).sum())            # flag 4 alone: the Planar items are skipped


# ---------------------------------------------------------------- 6. frame edges of the 4-tap block output
@TAP4_VARIANT
@pytest.mark.parametrize("size", V.EDGE_SIZES, ids=lambda s: "%dx%d" % tuple(s))
def test_frame_edge_residues(gpu_available, size, variant):
    """Every fifth size of tests/size_sweep.py, one noise frame, every 37th available CU, the modes
    of angular_tap4_cases.SWEEP_LIST cycling, against angular_tap4_ref.predict_cu.  The kernels cut a
    CU's table length to the samples left in row y - 1 / column x - 1 (`room`); at none of the 70
    sizes of the sweep does an available CU's table length exceed it
    (tests/test_predict_angular_variants_cpu.py test_no_table_length_exceeds_the_room), so there is
    no further size to run for ext4: the cut never changes a length the engine's own table gives."""
    w, h = size
    frame, un, cus, modes = V.edge_case(w, h)
    e_top, e_left = V.variant_lengths(variant, w, h)
    items, total = mipgpu.pred_items(w, h, 0, cus, BASE + modes)
    with _engine(w, h, variant) as eng:
        got, skipped = eng.predict(frame, items, total, angular=True)
    assert skipped == 0
    _, x, y, bw, bh = layout.cu_geometry(w, h, cus)
    at = 0
    for i, c in enumerate(cus):
        block = got[at:at + bw[i] * bh[i]].reshape(bh[i], bw[i])
        at += block.size
        want = V.block_of(variant, frame, x[i], y[i], bw[i], bh[i], e_top[c], e_left[c], int(modes[i]))
        assert np.array_equal(block, want), (int(c), int(modes[i]), int(e_top[c]), int(e_left[c]))
    assert at == total

