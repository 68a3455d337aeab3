"""Every partial-CTU frame-size residue through the HIP filters and the search
(tests/size_sweep.py: each nonzero W % 128 and H % 128 once in 2x2-CTU frames and once in
frames narrower than a CTU, plus residue 0 on one axis), bit for bit against the C oracle,
which tests/test_size_sweep_cpu.py ties to the reference's kernels at the same sizes.  What
depends on the residues: the linear addressing of the window and the reference lattice
(frame_chunk, WindowStager, stage_lattice), the CTU variants with their work and fill lists
(work_plan.h ctu_variants, cu_defined), the CUs of the exact per-CU kernel
(reads_last_columns), the unavailable CUs (filter_poison, reads_poison) and the filters'
per-tile halo gates (mip_filter.hip tap_valid, sep_fetch, inner_value)."""
import numpy as np
import pytest

import oracle_lib as O
import size_sweep as S
from mipgpu import MipEngine, filter_device, layout
from test_gpu_parity import FILTERS, _waves

pytestmark = pytest.mark.gpu

# (index in ALL_SIZES, family, index in the family, size)
SWEEP = [(n, fam, i, size) for n, (fam, i, size) in enumerate(
    [("A", i, s) for i, s in enumerate(S.FAMILY_A)] + [("B", i, s) for i, s in enumerate(S.FAMILY_B)] +
    [("C", i, s) for i, s in enumerate(S.FAMILY_C)])]


def _id(p):
    return "%s%02d-%s" % (p[1], p[2], S.size_id(p[3]))


@pytest.mark.parametrize("p", SWEEP, ids=_id)
def test_filters_at_every_residue(gpu_available, p):
    """All 28 (filter, kernel index) pairs on noise, bright edges, near-black and white frames:
    eng.filter_frames equals O.filter_frame.  On `edges` every separable filter must exceed
    1023 in the last columns where W % 128 != 0 (a condition on the input: the exact per-CU
    kernel then has something to do in test_search_at_every_residue)."""
    _, _, _, (w, h) = p
    frames = {kind: S.content(kind, w, h) for kind in S.CONTENTS}
    with MipEngine(w, h) as eng:  # refused at a sweep size: a failure
        for filt, nk in FILTERS:
            for k in range(nk):
                for kind, fr in frames.items():
                    want = O.filter_frame(fr, filt, k)
                    if kind == "edges" and filt in S.SEP and w % 128:
                        assert want.max() > 1023, (filt, k)
                    got = eng.filter_frames(fr, filt, k)[0]
                    assert np.array_equal(got, want), (filt, k, kind, np.argwhere(got != want)[:4])


def test_filter_frames_beyond_max_batch(gpu_available):
    """More frames than max_batch in one eng.filter_frames call (3 distinct frames on an engine
    of 2: a chunk of two and a chunk of one), with one separable and one 2-D filter: every
    frame of the output equals the oracle's filter of that frame."""
    w, h = 136, 72
    frames = np.stack([S.content("noise", w, h, salt) for salt in (0, 1, 2)])
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
    with MipEngine(w, h, max_batch=2) as eng:
        for filt in (S.SEP[0], S.TWO_D[0]):
            got = eng.filter_frames(frames, filt, 0)
            assert got.shape == frames.shape
            for f in range(3):
                assert np.array_equal(got[f], O.filter_frame(frames[f], filt, 0)), (filt, f)


# Widths that are no multiple of 4 (the engine refuses them, the module-level filter does not):
# the only ones at which a 2-D filter's left / right halo gate `qx + tc < W - 1` (tap_valid) has
# its boundary case qx + tc == W - 1 -- halo columns are qx + 128 and qx + 129 -- and, at
# W % 128 == 1, a last tile of one column, whose left halo the reference's separable 3-tap
# filter does not fetch (intra.cl:3351; sep_fetch had fetched it).
ODD_FILTER_SIZES = [(129, 36), (130, 40), (257, 68), (258, 36)]


@pytest.mark.parametrize("size", [s for _, _, _, s in SWEEP[::3]] + ODD_FILTER_SIZES, ids=S.size_id)
def test_filter_device_batches(gpu_available, size):
    """The module-level filter_device on 2-frame batches (noise, edges) and (noise, white):
    each frame equals the oracle's, and frame 0 does not change with what follows it."""
    import torch
    w, h = size
    noise, edges, white = (S.content(kind, w, h) for kind in ("noise", "edges", "white"))
    batches = [torch.from_numpy(np.stack(b).astype(np.int16)).cuda() for b in ((noise, edges), (noise, white))]
    for filt, nk in FILTERS:
        for k in range(nk):
            outs = [filter_device(b, torch.empty_like(b), filt, k) for b in batches]
            torch.cuda.synchronize()
            a, b = (o.cpu().numpy().view(np.uint16) for o in outs)
            assert np.array_equal(a[0], b[0]), (filt, k)
            assert np.array_equal(a[0], O.filter_frame(noise, filt, k)), (filt, k)
            assert np.array_equal(a[1], O.filter_frame(edges, filt, k)), (filt, k)
            assert np.array_equal(b[1], O.filter_frame(white, filt, k)), (filt, k)


def _decisions_only(eng, d, refs=None):
    """Decisions-only device search into outputs prefilled with a sentinel (an entry nobody
    writes fails), as test_device_decisions_only_fused_argmin."""
    import torch
    n = d.shape[0]
    bm = torch.full((n, eng.cus_per_frame), 0x5a, dtype=torch.uint8, device="cuda")
    bc = torch.full((n, eng.cus_per_frame), -5, dtype=torch.int32, device="cuda")
    assert eng.search_device(d, refs=refs, costs=False, best_mode=bm, best_cost=bc) is None
    torch.cuda.synchronize()
    eng.check_input()
    return bm.cpu().numpy(), bc.cpu().numpy()


def _assert_tables(out, dec, want, nct, tag):
    """Engine tables `out` and decisions-only lists `dec` of a batch against the oracle's
    (cost, sad, satd) per frame."""
    for f, (oc, osad, osatd) in enumerate(want):
        for key, o in (("cost", oc), ("sad", osad), ("satd", osatd)):
            bad = np.nonzero(out[key][f] != o)[0]
            assert bad.size == 0, (tag, key, f, bad.size, bad[:4], out[key][f][bad[:4]], o[bad[:4]])
        bm, bc = layout.best_modes(oc, nct)
        assert np.array_equal(out["best_mode"][f], bm), (tag, f)
        assert np.array_equal(out["best_cost"][f], bc), (tag, f)
        assert np.array_equal(dec[0][f], bm), (tag, "decisions only", f, np.nonzero(dec[0][f] != bm)[0][:4])
        assert np.array_equal(dec[1][f], bc), (tag, "decisions only", f, np.nonzero(dec[1][f] != bc)[0][:4])


def _sweep_filters(n, fam, i):
    """The engine filters of sweep size n: one separable filter, and for every second size of
    family A and all of B and C one 2-D filter too."""
    filts = [(S.SEP[n % 4], n % 3)]
    if fam != "A" or i % 2 == 0:
        filts.append((S.TWO_D[n % 4], n % 3))
    return filts


@pytest.mark.parametrize("p", SWEEP, ids=_id)
def test_search_at_every_residue(gpu_available, p):
    """A 2-frame batch of `edges` frames: original references, the engine's filter (one
    separable -- samples above 1023 in the last columns: the exact per-CU kernel -- and mostly
    one 2-D) and caller references with columns W-2, W-1 above 1023: cost / SAD / SATD tables,
    the UNAVAILABLE set and the decisions (with the table and decisions only) equal the
    oracle's on every entry."""
    import torch
    n, fam, i, (w, h) = p
    nct = layout.num_ctus(w, h)
    frames = np.stack([S.content("edges", w, h, salt) for salt in (0, 1)])
    refs = np.stack([S.caller_refs(w, h, salt) for salt in (0, 1)])
    assert (refs.max() > 1023) == (w % 128 != 0)
    d = torch.from_numpy(frames.astype(np.int16)).cuda()
    dr = torch.from_numpy(refs.astype(np.int16)).cuda()
    with MipEngine(w, h, max_batch=2, want_sad_satd=True) as eng:
        out = eng.search(frames, best=True, sad_satd=True)
        dec = _decisions_only(eng, d)
        out_r = eng.search(frames, refs=refs, best=True, sad_satd=True)
        dec_r = _decisions_only(eng, d, dr)
    want = [O.search(frames[f], want_sad_satd=True) for f in range(2)]
    _assert_tables(out, dec, want, nct, "original references")
    avail = layout.available_mask(w, h)
    for f in range(2):
        assert np.array_equal(out["cost"][f] == layout.UNAVAILABLE, ~avail), f
    want = [O.search(frames[f], refs[f], want_sad_satd=True) for f in range(2)]
    _assert_tables(out_r, dec_r, want, nct, "caller references")
    for filt, k in _sweep_filters(n, fam, i):
        with MipEngine(w, h, max_batch=2, filter=filt, kernel_idx=k, want_sad_satd=True) as eng:
            out = eng.search(frames, best=True, sad_satd=True)
            dec = _decisions_only(eng, d)
        want = [O.engine_search(frames[f], filt, k, want_sad_satd=True) for f in range(2)]
        _assert_tables(out, dec, want, nct, (filt, k))
        for f in range(2):
            unav = O.engine_unavailable_mask(frames[f], filt, k)
            assert np.array_equal(out["cost"][f] == layout.UNAVAILABLE, unav), (filt, k, f)


@pytest.mark.parametrize("waves,pk", [(12, "0"), (8, "8")])
@pytest.mark.parametrize("p", [q for q in SWEEP if q[1] in "AB" and q[2] % 4 == 0], ids=_id)
def test_other_kernel_designs_at_residues(gpu_available, monkeypatch, p, waves, pk):
    """Small launches run the 16-wave kernel by default (test_search_at_every_residue).  Every
    fourth size of families A and B also goes through the 12-wave kernel (MIPGPU_WIDE=0,
    MIPGPU_PIPE_KERNEL=0) and the four-wave twin (MIPGPU_PIPE_KERNEL=8) -- the census proves
    it -- with the size's separable filter: tables, and decisions only into prefilled outputs."""
    monkeypatch.setenv("MIPGPU_WIDE", "0")
    monkeypatch.setenv("MIPGPU_PIPE_KERNEL", pk)
    n, fam, i, (w, h) = p
    filt, k = _sweep_filters(n, fam, i)[0]
    nct = layout.num_ctus(w, h)
    frames = np.stack([S.content("edges", w, h, salt) for salt in (0, 1)])
    with MipEngine(w, h, max_batch=2, filter=filt, kernel_idx=k, want_sad_satd=True) as eng:
        out = eng.search(frames, best=True, sad_satd=True)
        pre = {"best_mode": np.full((2, eng.cus_per_frame), 0x5a, np.uint8),
               "best_cost": np.full((2, eng.cus_per_frame), -5, np.int32)}
        dec = eng.search(frames, costs=False, best=True, out=pre)
        census = eng.search_census()
    assert _waves(census) == {waves}, census
    want = [O.engine_search(frames[f], filt, k, want_sad_satd=True) for f in range(2)]
    _assert_tables(out, (dec["best_mode"], dec["best_cost"]), want, nct, (filt, k, waves))
