"""Every partial-CTU frame-size residue (tests/size_sweep.py, 70 sizes) through the kernels that
came after the filter / search sweep: intra_kernel (Planar / DC tables, the merge),
partition_kernel and, in a device chain, mip_predict -- bit for bit against the restatements
(tests/intra_ref.py, tests/partition_ref.py, tests/predict_ref.py; inputs and references in
tests/edge_sweep_cases.py).  What depends on W % 128, H % 128 and W % 32 here: the 32x32 / 64x64
window staged by linear index with wrap, CUs right of the frame, the availability sets of the
reference source (all eight engine filters), the partition's "outside the frame costs 0" rule
and its leaf rule x + w <= W.

The CPU tests (not `gpu`) show that what the GPU tests assert about their inputs holds for the
references alone: a GPU failure then means the kernel."""
import numpy as np
import pytest

import edge_sweep_cases as E
import intra_ref as I
import mipgpu
import partition_cases as C
import size_sweep as S
from mipgpu import MipEngine, layout

gpu = pytest.mark.gpu
UN = layout.UNAVAILABLE

# (family, index in the family, size), literal sizes as tests/test_gpu_size_sweep.py
SWEEP = ([("A", i, s) for i, s in enumerate(S.FAMILY_A)] + [("B", i, s) for i, s in enumerate(S.FAMILY_B)] +
         [("C", i, s) for i, s in enumerate(S.FAMILY_C)])
FIFTH = SWEEP[::5]
# one CTU without a partition per family: (size, CTU); the 4x4 at (20, 36) of that CTU is in the frame
HOLES = [("A", 4, (148, 148), 0), ("B", 19, (80, 196), 0), ("C", 0, (256, 132), 1)]
# the engine filters of the filter sweep: two on every fifth size, the other six once at 136x72
FILTER_CASES = ([(p, f) for p in FIFTH for f in (E.FILTER_SEP, E.FILTER_2D)] +
                [(("-", 0, E.OTHER_SIZE), f) for f in E.OTHER_FILTERS])


def _id(p):
    return "%s%02d-%s" % (p[0], p[1], S.size_id(p[2]))


# ---------------------------------------------------------------- CPU: the inputs' conditions
def test_sweep_sizes_and_filters():
    assert [s for _, _, s in SWEEP] == S.ALL_SIZES and len(SWEEP) == 70 and len(FIFTH) == 14
    assert {f for f, _, _ in FIFTH} == {"A", "B", "C"}
    assert sorted(E.OTHER_FILTERS + [E.FILTER_SEP, E.FILTER_2D]) == sorted(mipgpu.FILTERS)
    assert E.FILTER_SEP in S.SEP and E.FILTER_2D in S.TWO_D
    assert len(set(E.VECTOR_PENALTY)) == layout.NUM_SHAPES and max(E.VECTOR_PENALTY) <= mipgpu.PART_MAX_PENALTY
    for fam, i, size, ctu in HOLES:
        assert (fam, i, size) in SWEEP and size[0] > 128 * (ctu % 2) + 20 and size[1] > 36 and ctu < layout.ctu_grid(*size)[0]
        assert layout.num_ctus(*size) >= 2                    # another CTU keeps its partition


def test_available_and_wrapped_cus_at_every_size():
    """Available CUs exist at every size; where W % 128 != 0 some of them reach past the right
    edge (their windows wrap into the next rows) -- at every size but 124x4; every filter's availability set at the sizes
    it runs on leaves CUs available and takes some away (or none: a 2-D filter at 128-multiples)."""
    for w, h in S.ALL_SIZES:
        un = mipgpu.unavailable_cus(w, h)
        assert (~un).any() and un.any() == bool(w % 128 or h % 128), (w, h)
        if w % 128:                                           # (124x4: one row of 4x4 CUs, a wrapped one would read past the end)
            assert (~un & E.wrapped(w, h)).any() == ((w, h) != (124, 4)), (w, h)
    sets = set()
    for (_, _, (w, h)), filt in FILTER_CASES:
        un, base = mipgpu.unavailable_cus(w, h, filt), mipgpu.unavailable_cus(w, h)
        assert (~un).any() and (un >= base).all(), (w, h, filt)
        if (w, h) == E.OTHER_SIZE:
            sets.add(un.tobytes())
    assert len(sets) > 1                                      # the filters' sets at 136x72 are not all one set


def test_clip_is_reachable_with_the_separable_filter():
    """`edges` frames through a separable filter: where W % 128 != 0 an available CU has a
    boundary sample above 1023, so the PDPC clip fires."""
    for (_, _, (w, h)), filt in FILTER_CASES:
        _, refs, un, _ = E.intra_case(w, h, "edges", filt)
        if filt in S.SEP and w % 128:
            assert E.max_boundary(refs, un, w, h) > 1023, (w, h, filt)


def test_partition_sweep_inputs_have_a_partition():
    """The Planar / DC minimum costs give every CTU of every sweep size a partition (which is why
    the sweep adds the HOLES cases), with leaves of more than one shape."""
    for w, h in S.ALL_SIZES:
        cost, mode, ref = E.partition_case(w, h)
        assert (ref["ctu_cost"] != UN).all() and (ref["ctu_leaves"] > 0).all(), (w, h)
        assert set(np.unique(mode)) <= {I.MODE_PLANAR, I.MODE_DC, 0xFF}
    for _, _, (w, h), ctu in HOLES:
        ref = C.reference(w, h, "holes", C.MID_PENALTY, 1, ctu)
        assert ref["ctu_cost"][0, ctu] == UN and (np.delete(ref["ctu_cost"][0], ctu) != UN).all(), (w, h)


def test_chain_inputs_mix_mip_planar_and_dc():
    """Over the chain's sizes Planar, DC and MIP modes all win CUs and all are leaves; at every
    size the partition has MIP leaves and, but at 20x20 (13 leaves), regular ones."""
    won, leaves = set(), set()
    for _, _, (w, h) in FIFTH:
        c = E.chain_case(w, h)
        assert (c["ctu_cost"] != UN).all(), (w, h)
        assert (c["leaf"] & ~c["regular"]).any() and c["regular"].any() == ((w, h) != (20, 20)), (w, h)
        assert (c["canvas"] == E.FILL).any() == c["regular"].any() and (c["canvas"] <= 1023).any(), (w, h)
        won |= set(np.unique(c["best_mode"]))
        leaves |= set(np.unique(c["best_mode"][0, c["leaf"]]))
    for s in (won, leaves):
        assert I.MODE_PLANAR in s and I.MODE_DC in s and any(m < 32 for m in s)


# ---------------------------------------------------------------- GPU
def _intra_tables(eng, frame):
    from test_gpu_intra import Arena, _dev
    arena = Arena(1, eng.cus_per_frame)
    eng.intra_device(_dev(frame[None]), **{k: arena.tensor(k) for k in E.TABLES})
    return arena.read(E.TABLES)


def _assert_tables(got, tabs, un, tag):
    for key in E.TABLES:
        bad = np.nonzero((got[key][0] != tabs[key]).any(axis=1))[0]
        assert bad.size == 0, (tag, key, bad.size, bad[:4], got[key][0][bad[:4]], tabs[key][bad[:4]])
        assert np.array_equal(got[key][0, :, 0] == UN, un) and np.array_equal(got[key][0, :, 1] == UN, un), (tag, key)


@gpu
@pytest.mark.parametrize("p", SWEEP, ids=_id)
def test_intra_at_every_residue(gpu_available, p):
    """One noise frame, original references: the three tables and the UNAVAILABLE pattern."""
    w, h = p[2]
    frame, _, un, tabs = E.intra_case(w, h)
    assert np.array_equal(un, mipgpu.unavailable_cus(w, h)) and (~un).any()
    if w % 128 and (w, h) != (124, 4):
        assert (~un & E.wrapped(w, h)).any()
    with MipEngine(w, h) as eng:                              # refused at a sweep size: a failure
        got, clean = _intra_tables(eng, frame)
    assert clean
    _assert_tables(got, tabs, un, (w, h))


def _partition(cost, mode, w, h, penalty):
    from test_gpu_partition import _partition, _same
    got, clean = _partition(cost, mode, w, h, penalty)
    assert clean
    return got, _same


@gpu
@pytest.mark.parametrize("p", SWEEP, ids=_id)
def test_partition_at_every_residue(gpu_available, p):
    """Costs made on the host from the size's Planar / DC reference, a penalty per shape: all
    four outputs, padding and legality."""
    w, h = p[2]
    cost, mode, ref = E.partition_case(w, h)
    assert (ref["ctu_cost"] != UN).all()
    got, same = _partition(cost, mode, w, h, E.VECTOR_PENALTY)
    same(got, ref, w, h)


@gpu
@pytest.mark.parametrize("p", HOLES, ids=_id)
def test_partition_without_a_partition_at_odd_sizes(gpu_available, p):
    """Synthetic costs with holes and one CTU that cannot be tiled, one size per family."""
    _, _, (w, h), ctu = p
    cost, mode = C.impossible(w, h, ctu)
    ref = C.reference(w, h, "holes", C.MID_PENALTY, 1, ctu)
    got, same = _partition(cost, mode, w, h, C.MID_PENALTY)
    same(got, ref, w, h)
    assert got["ctu_cost"][0, ctu] == UN and got["ctu_leaves"][0, ctu] == 0 and (got["ctu_cost"] != UN).any()


@gpu
@pytest.mark.parametrize("case", FILTER_CASES, ids=lambda c: _id(c[0]) + "-" + c[1][len("filterFrame_"):])
def test_intra_with_engine_filters(gpu_available, case):
    """`edges` frames, the engine filters the references itself: tables and UNAVAILABLE pattern
    against the restatement on the oracle's filtered frame with that filter's availability set."""
    (_, _, (w, h)), filt = case
    frame, refs, un, tabs = E.intra_case(w, h, "edges", filt)
    if filt in S.SEP and w % 128:                             # the clip is exercised
        assert E.max_boundary(refs, un, w, h) > 1023
    with MipEngine(w, h, filter=filt) as eng:
        got, clean = _intra_tables(eng, frame)
    assert clean
    _assert_tables(got, tabs, un, (w, h, filt))


@gpu
@pytest.mark.parametrize("p", FIFTH, ids=_id)
def test_chain_at_every_fifth_size(gpu_available, p):
    """search_device (decisions only, outputs prefilled) -> intra_device merge -> partition_device
    -> predict_device into a frame canvas, no host round trip."""
    import torch
    from test_gpu_intra import _dev
    from test_gpu_partition import OUTPUTS, Arena
    w, h = p[2]
    want = E.chain_case(w, h)
    with MipEngine(w, h) as eng:
        nct, ncu = eng.nctus, eng.cus_per_frame
        d_frames = _dev(want["frame"][None])
        bm = torch.full((1, ncu), 0x5A, dtype=torch.uint8, device="cuda")
        bc = torch.full((1, ncu), -3, dtype=torch.int32, device="cuda")
        assert eng.search_device(d_frames, costs=False, best_mode=bm, best_cost=bc) is None
        mip_mode, mip_cost = bm.cpu().numpy(), bc.cpu().numpy()
        eng.intra_device(d_frames, bias=E.CHAIN_BIAS, best_mode=bm, best_cost=bc)
        arena = Arena(1, nct)
        mipgpu.partition_device(bc, w, h, penalty=E.CHAIN_PENALTY, best_mode=bm, **{k: arena.tensor(k) for k in OUTPUTS})
        canvas = torch.full((w * h + 64,), -1, dtype=torch.int16, device="cuda")
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.predict_device(d_frames, arena.tensor("items"), canvas[:w * h], skipped=sk)
        eng.check_input()
        got, clean = arena.read(OUTPUTS)
    assert clean
    assert np.array_equal(mip_mode, want["mip_mode"]) and np.array_equal(mip_cost, want["mip_cost"])
    assert np.array_equal(bm.cpu().numpy(), want["best_mode"]) and np.array_equal(bc.cpu().numpy(), want["best_cost"])
    assert np.array_equal(got["leaf"][0].astype(bool), want["leaf"])
    for key in ("ctu_cost", "ctu_leaves", "items"):
        assert np.array_equal(got[key], want[key]), key
    C.check_legal(got["leaf"], got["ctu_cost"], got["ctu_leaves"], w, h)
    # every MIP leaf's block is predict_ref's, the regular leaves' samples and the tail stay unwritten
    samples = canvas.cpu().numpy().view(np.uint16)
    bad = np.argwhere(samples[:w * h].reshape(h, w) != want["canvas"])
    assert bad.size == 0, (len(bad), bad[:4])
    assert np.all(samples[w * h:] == E.FILL)
    padding = nct * mipgpu.PART_MAX_LEAVES - int(got["ctu_leaves"].sum())
    assert int(sk.item()) == padding + int(want["regular"].sum())
