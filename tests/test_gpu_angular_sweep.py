"""Every partial-CTU frame-size residue (tests/size_sweep.py, 70 sizes) through angular_kernel
(mip_angular_device / mip_angular_frames), bit for bit against the numpy restatement
tests/angular_ref.py (pinned by tests/test_angular_cpu.py; inputs and references in
tests/edge_sweep_cases.py).  What depends on W % 128, H % 128 and on how a 32x32 or 64x64 window
wraps over several frame rows, and that the intra kernel never does: the corner sample (s_left[0]
or window row -1, or its top[0] substitute), the boundary lines as base + stride of the staged
window (stride 0 and the constant cell on the first frame row and column), the side projection of
the negative angles up to its cap S, the 64x64 path's availability per quadrant, all eight engine
filters' references, and the host call's 256 MiB table cut.

The CPU tests (not `gpu`) show that what the GPU tests need of their inputs holds for the
references alone: a GPU failure then means the kernel."""
import numpy as np
import pytest

import angular_ref as A
import edge_sweep_cases as E
import intra_ref as I
import mipgpu
import partition_cases as C
import size_sweep as S
from mipgpu import MipEngine, layout
from test_gpu_edge_sweep import FIFTH, FILTER_CASES, SWEEP, _id

gpu = pytest.mark.gpu
UN = layout.UNAVAILABLE
PAIR = ("ang_mode", "ang_cost")
ALL_OUT = E.TABLES + PAIR
TABLE_BYTES = 256 << 20                                       # kAngularTableBytes of mip_angular_frames
CUT_SIZE, CUT_FRAMES, CUT_PERIOD, CUT_MODES = (60, 52), 200, 3, (18, 34, 50)


def _listed(modes):
    listed = np.zeros(A.MODES, bool)
    listed[np.array(A.ALL_MODES if modes is None else modes) - A.FIRST] = True
    return listed


# ---------------------------------------------------------------- CPU: the inputs' conditions
def test_sweep_modes_cover_both_classes_and_the_angle_extremes():
    modes, angle = E.SWEEP_MODES, A.ANGLE
    assert len(modes) % 2 == 1 and list(modes) == sorted(set(modes))    # the last round of two modes is half empty
    hor, ver = [m for m in modes if m < 34], [m for m in modes if m >= 34]
    assert 18 in hor and 50 in ver and angle[18] == 0 == angle[50]      # both pure modes (PDPC)
    assert any(angle[m] == 32 for m in hor) and any(angle[m] == 32 for m in ver)
    assert any(angle[m] == -32 for m in modes)                          # the diagonal
    assert any(angle[m] == -1 for m in modes) and any(angle[m] == 1 for m in modes)
    assert any(angle[m] == -29 for m in hor) and any(angle[m] == -29 for m in ver)
    for cls in (hor, ver):
        assert any(angle[m] < 0 for m in cls) and any(angle[m] > 0 for m in cls)
    assert [s for _, _, s in SWEEP] == S.ALL_SIZES and len(SWEEP) == 70 and len(FIFTH) == 14 and len(FILTER_CASES) == 34


def test_available_cus_on_the_first_row_and_column_at_every_size():
    """Available CUs exist at every size; where W % 128 != 0 one of them reaches past the right
    edge (but at 124x4); wherever the frame has more than one CU row (column) an available CU sits
    in the first column below the first row (in the first row right of the first column): the
    stride-0 lines and the substituted corner."""
    for w, h in S.ALL_SIZES:
        un = mipgpu.unavailable_cus(w, h)
        x, y, _, _ = E.geometry(w, h)
        ok = ~un
        assert ok.any(), (w, h)
        if w % 128:
            assert (ok & E.wrapped(w, h)).any() == ((w, h) != (124, 4)), (w, h)
        assert (ok & (x == 0) & (y == 0)).any(), (w, h)
        if h > 4:
            assert (ok & (x == 0) & (y > 0)).any(), (w, h)
        if w > 4:
            assert (ok & (y == 0) & (x > 0)).any(), (w, h)


def test_pdpc_leaves_the_sample_range_on_the_noise_frames():
    """Before the clip, modes 18 and 50 fall below 0 and rise above 1023 on available CUs of the
    noise sweep: at 148x148 and at 20x20 alone, and so over the sweep as a whole -- not at 124x4
    (one CU row: every top line is a substitute), which therefore does not count."""
    lo, hi = {}, {}
    for w, h in S.ALL_SIZES:
        _, refs, un, _ = E.intra_case(w, h)
        lo[w, h], hi[w, h] = E.pdpc_range(refs, un, w, h)
    assert min(lo.values()) < 0 and max(hi.values()) > 1023
    for size in ((148, 148), (20, 20)):
        assert lo[size] < 0 and hi[size] > 1023, (size, lo[size], hi[size])
    assert lo[124, 4] >= 0 and hi[124, 4] <= 1023


def test_filtered_boundaries_or_corners_exceed_the_sample_range():
    """`edges` frames through a separable filter: where W % 128 != 0 the largest boundary or corner
    sample of an available CU exceeds 1023 (32-bit arithmetic and the clip are exercised).  The
    2-D filters stay within 10 bits, which is expected and not asserted."""
    seen = 0
    for (_, _, (w, h)), filt in FILTER_CASES:
        if filt in S.SEP and w % 128:
            _, refs, un, _ = E.intra_case(w, h, "edges", filt)
            assert E.max_boundary_or_corner(refs, un, w, h) > 1023, (w, h, filt)
            seen += 1
    assert seen >= 13


def test_projection_reaches_its_cap_and_the_corner():
    """Over the sweep the side projection of a negative angle reaches its cap (p >= S, the read of
    side'[S]) on an available CU in both classes, and the corner (ref[0]) is read in both.  A
    negative k never projects onto the corner: the smallest inverse angle is 512, so
    p = (-k * inv + 256) >> 9 >= 1 there -- p == 0 occurs at k == 0 only."""
    assert min(A.INVERSE.values()) == 512 and (1 * 512 + 256) >> 9 == 1
    cap, corner = set(), set()
    for w, h in S.ALL_SIZES:
        un = mipgpu.unavailable_cus(w, h)
        shape = layout.cu_geometry(w, h, np.nonzero(~un)[0])[0]
        for s in (layout.SHAPES[i] for i in np.unique(shape)):
            for m in (m for m in E.SWEEP_MODES if A.ANGLE[m] < 0):
                k, p, side = E.projection(s.w, s.h, m)
                assert np.all(p[k < 0] >= 1)
                if (p[k < 0] >= side).any():
                    cap.add(m >= 34)
                if (k == 0).any():
                    corner.add(m >= 34)
    assert cap == {False, True} and corner == {False, True}


def test_angular_chain_inputs_mix_all_three_kinds():
    """Over the chain's sizes MIP, Planar / DC and angular modes all win CUs and all are leaves."""
    won, leaves = np.zeros(3, int), np.zeros(3, int)
    for _, _, (w, h) in FIFTH:
        c = E.angular_chain_case(w, h)
        assert (c["ctu_cost"] != UN).all(), (w, h)
        mode = c["best_mode"][0]
        kinds = [mode < 32, (mode == I.MODE_PLANAR) | (mode == I.MODE_DC), (mode >= A.MODE_BASE + A.FIRST) & (mode <= A.MODE_BASE + A.LAST)]
        won += [int(k.sum()) for k in kinds]
        leaves += [int(c[k].sum()) for k in ("mip", "regular", "angular")]
        assert np.array_equal(c["leaf"], c["mip"] | c["regular"] | c["angular"])
        assert (c["canvas"] == E.FILL).any() == c["angular"].any(), (w, h)
    assert won.all() and leaves.all(), (won, leaves)
    assert not np.array_equal(E.angular_chain_case(136, 188)["best_mode"], E.chain_case(136, 188)["best_mode"])


def test_the_table_cut_falls_inside_the_call():
    chunk = _cut_chunk()
    assert chunk == 191 and chunk < CUT_FRAMES and chunk % CUT_PERIOD and CUT_SIZE in S.ALL_SIZES and layout.num_ctus(*CUT_SIZE) == 1


def _cut_chunk():
    return TABLE_BYTES // (layout.num_ctus(*CUT_SIZE) * layout.CUS_PER_CTU * A.MODES * 4)


# ---------------------------------------------------------------- GPU
def _run(eng, frame, modes, given=ALL_OUT):
    from test_gpu_angular import _run
    return _run(eng, frame[None], modes=modes, given=given)


def _assert_same(got, want, un, modes, tag):
    """Every output of `got` (one frame) equals `want`; the UNAVAILABLE pattern of the tables."""
    listed = _listed(modes)
    for key in got:
        g, t = got[key][0], want[key]
        bad = np.nonzero((g != t).reshape(un.size, -1).any(axis=1))[0]
        assert bad.size == 0, (tag, key, bad.size, bad[:4], g[bad[:4]], t[bad[:4]])
        if key in E.TABLES:
            assert np.array_equal(g[:, listed] == UN, np.broadcast_to(un[:, None], (un.size, int(listed.sum())))), (tag, key)
            assert np.all(g[:, ~listed] == UN), (tag, key)
    if "ang_cost" in got:
        assert np.array_equal(got["ang_cost"][0] == UN, un) and np.array_equal(got["ang_mode"][0] == 0xFF, un), tag


@gpu
@pytest.mark.parametrize("p", SWEEP, ids=_id)
def test_angular_at_every_residue(gpu_available, p):
    """One noise frame, original references, SWEEP_MODES: the three tables, the ang pair and the
    UNAVAILABLE pattern."""
    w, h = p[2]
    frame, _, un, tabs = E.angular_sweep_case(w, h)
    assert np.array_equal(un, mipgpu.unavailable_cus(w, h)) and (~un).any()
    with MipEngine(w, h) as eng:
        got, clean = _run(eng, frame, E.SWEEP_MODES)
    assert clean
    _assert_same(got, tabs, un, E.SWEEP_MODES, (w, h))


@gpu
@pytest.mark.parametrize("p", FIFTH, ids=_id)
def test_angular_all_modes_at_every_fifth_size(gpu_available, p):
    """All 65 modes: every slot of the cost table and the ang pair; at the sizes of more than one
    CTU most modes win somewhere."""
    w, h = p[2]
    frame, _, un, tabs = E.angular_sweep_case(w, h, modes=None)
    given = ("cost",) + PAIR
    with MipEngine(w, h) as eng:
        got, clean = _run(eng, frame, None, given)
    assert clean
    _assert_same(got, {k: tabs[k] for k in given}, un, None, (w, h))
    if layout.num_ctus(w, h) > 1:
        assert len(np.unique(got["ang_mode"])) > 40


@gpu
@pytest.mark.parametrize("case", FILTER_CASES, ids=lambda c: _id(c[0]) + "-" + c[1][len("filterFrame_"):])
def test_angular_with_engine_filters(gpu_available, case):
    """`edges` frames, the engine filters the references itself: tables, pair and UNAVAILABLE
    pattern against the restatement on the oracle's filtered frame with that filter's set."""
    (_, _, (w, h)), filt = case
    frame, refs, un, tabs = E.angular_sweep_case(w, h, "edges", filt)
    if filt in S.SEP and w % 128:
        assert E.max_boundary_or_corner(refs, un, w, h) > 1023
    with MipEngine(w, h, filter=filt) as eng:
        got, clean = _run(eng, frame, E.SWEEP_MODES)
    assert clean
    _assert_same(got, tabs, un, E.SWEEP_MODES, (w, h, filt))


@gpu
@pytest.mark.parametrize("p", FIFTH, ids=_id)
def test_angular_chain_at_every_fifth_size(gpu_available, p):
    """search_device (decisions only, outputs prefilled) -> intra_device merge -> angular_device
    merge -> partition_device -> predict_device(regular=True) into a frame canvas, no host round
    trip: angular leaves and the tail stay unwritten."""
    import torch
    from test_gpu_intra import _dev
    from test_gpu_partition import OUTPUTS, Arena
    w, h = p[2]
    want = E.angular_chain_case(w, h)
    with MipEngine(w, h) as eng:
        nct, ncu = eng.nctus, eng.cus_per_frame
        d_frames = _dev(want["frame"][None])
        bm = torch.full((1, ncu), 0x5A, dtype=torch.uint8, device="cuda")
        bc = torch.full((1, ncu), -3, dtype=torch.int32, device="cuda")
        assert eng.search_device(d_frames, costs=False, best_mode=bm, best_cost=bc) is None
        mip_mode, mip_cost = bm.cpu().numpy(), bc.cpu().numpy()
        eng.intra_device(d_frames, bias=E.CHAIN_BIAS, best_mode=bm, best_cost=bc)
        intra_mode, intra_cost = bm.cpu().numpy(), bc.cpu().numpy()
        assert eng.angular_device(d_frames, modes=E.SWEEP_MODES, bias=E.ANGULAR_CHAIN_BIAS, best_mode=bm, best_cost=bc) is None
        arena = Arena(1, nct)
        mipgpu.partition_device(bc, w, h, penalty=E.CHAIN_PENALTY, best_mode=bm, **{k: arena.tensor(k) for k in OUTPUTS})
        canvas = torch.full((w * h + 64,), -1, dtype=torch.int16, device="cuda")
        sk = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.predict_device(d_frames, arena.tensor("items"), canvas[:w * h], skipped=sk, regular=True)
        eng.check_input()
        got, clean = arena.read(OUTPUTS)
    assert clean
    assert np.array_equal(mip_mode, want["mip_mode"]) and np.array_equal(mip_cost, want["mip_cost"])
    assert np.array_equal(intra_mode, want["intra_mode"]) and np.array_equal(intra_cost, want["intra_cost"])
    mode, cost = bm.cpu().numpy(), bc.cpu().numpy()
    bad = np.nonzero((mode[0] != want["best_mode"][0]) | (cost[0] != want["best_cost"][0]))[0]
    assert bad.size == 0, ((w, h), bad.size, bad[:4], mode[0, bad[:4]], want["best_mode"][0, bad[:4]], cost[0, bad[:4]],
                           want["best_cost"][0, bad[:4]])
    assert np.array_equal(got["leaf"][0].astype(bool), want["leaf"])
    for key in ("ctu_cost", "ctu_leaves", "items"):
        assert np.array_equal(got[key], want[key]), key
    C.check_legal(got["leaf"], got["ctu_cost"], got["ctu_leaves"], w, h)
    samples = canvas.cpu().numpy().view(np.uint16)
    bad = np.argwhere(samples[:w * h].reshape(h, w) != want["canvas"])
    assert bad.size == 0, (len(bad), bad[:4])
    assert np.all(samples[w * h:] == E.FILL)
    padding = nct * mipgpu.PART_MAX_LEAVES - int(got["ctu_leaves"].sum())
    assert int(sk.item()) == padding + int(want["angular"].sum())


@gpu
def test_host_table_call_crosses_the_256_mib_cut(gpu_available):
    """200 frames of period 3 at 60x52 on max_batch = 200: with the table the chunk is cut to 191
    frames (256 MiB of 5380 x 65 x 4 B tables), so a second chunk of 9 frames follows at a frame
    index that is no multiple of the period; without the table the call is one chunk of 200."""
    w, h = CUT_SIZE
    chunk = _cut_chunk()
    assert chunk < CUT_FRAMES and chunk % CUT_PERIOD and CUT_FRAMES % CUT_PERIOD
    un = mipgpu.unavailable_cus(w, h)
    base = np.stack([S.content("noise", w, h, salt) for salt in range(CUT_PERIOD)])
    ref = [A.tables(f, f, un, CUT_MODES)["cost"] for f in base]
    best = [A.best(t) for t in ref]
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[1], ref[2]) and not np.array_equal(ref[0], ref[2])
    frames = base[np.arange(CUT_FRAMES) % CUT_PERIOD]
    with MipEngine(w, h, max_batch=CUT_FRAMES) as eng:
        host = eng.angular(frames, modes=CUT_MODES, table=True)
        pair = eng.angular(frames, modes=CUT_MODES)
    assert sorted(pair) == sorted(PAIR) and host["cost"].shape == (CUT_FRAMES, un.size, A.MODES)
    for f in range(CUT_FRAMES):                               # (frame by frame: no second copy of the table)
        q = f % CUT_PERIOD
        assert np.array_equal(host["cost"][f], ref[q]), ("cost", f, chunk)
        for res, tag in ((host, "table"), (pair, "pair")):
            assert np.array_equal(res["ang_mode"][f], best[q][0]) and np.array_equal(res["ang_cost"][f], best[q][1]), (tag, f, chunk)
