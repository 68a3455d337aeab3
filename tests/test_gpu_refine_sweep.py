"""Every partial-CTU frame-size residue (tests/size_sweep.py, 70 sizes) through
angular_refine_kernel (mip_angular_refine_device), the two host calls that were never run across
their 256 MiB table cut (mip_angular_refine_frames, mip_candidates_frames) and the candidate chain
of mip_candidates_frames at every fifth size -- bit for bit against the numpy restatements
(tests/angular_ref.py -> tests/angular_refine_ref.py, tests/intra_ref.py, tests/candidates_ref.py)
and the C oracle; inputs and references in tests/edge_sweep_cases.py.

What the refined kernel has that the swept angular_kernel has not: a refinement pass in which sample
values choose the mode each 16-lane group runs, so the class, angle-sign and PDPC branches diverge
inside a wave over boundary lines that are base + stride * t (stride 0 and the constant cell on the
first row and column); a 64x64 path that forms seeds and candidates on one lane, for CUs that may
be unavailable; and `tried`.  Seven (list, seeds) configurations rotate over the sizes, lists of
one and of two modes among them; a further one makes both PDPC modes candidates on the substituted
boundaries of the CUs at (0, 0).

The CPU tests (not `gpu`) show that the inputs reach what the GPU tests are about, for the
restatement alone: a GPU failure then means the kernel or the host walk."""
from functools import lru_cache

import numpy as np
import pytest

import angular_ref as A
import angular_refine_ref as RR
import edge_sweep_cases as E
import mipgpu
import size_sweep as S
from mipgpu import MipEngine, layout
from test_gpu_angular_refine import ALL_OUT, Arena, _dev
from test_gpu_edge_sweep import FIFTH, FILTER_CASES, SWEEP, _id

gpu = pytest.mark.gpu
slow = pytest.mark.slow
UN = layout.UNAVAILABLE
MERGE_BIAS = 9
# Floors of the counted conditions over the 70 sizes, well below what the rotation gives (82, 2756,
# 144 398, 8946 and 18 007 CUs; 161 and 337 CUs, 61 sizes, 47 016 CUs): the others must occur.
FLOORS = {"pdpc_first_column": 30, "pdpc_first_row": 1000, "wins_wrapped": 50000, "wins_first_column": 3000, "wins_first_row": 6000,
          "big_full": 1, "big_fewer": 1, "big_mixed_sizes": 1, "end_candidates": 1}
CALLER_REFS_CASE = ((192, 208), E.FILTER_SEP)                 # W % 128 == 64: wrapped CUs; one of FILTER_CASES
CHAIN_FILTERS = (None, E.FILTER_SEP, E.FILTER_2D)


def _filter_id(f):
    return "orig" if f is None else f[len("filterFrame_"):]


# ---------------------------------------------------------------- CPU: the inputs' conditions
def test_rotation_lists():
    """The rotation as the sweep needs it: seven entries, every one met by ten sizes; a list of one
    mode with one seed (nmodes == nseeds, a coarse round of two modes that is half empty); with
    (2, 66) every candidate is 3 or 65; the PDPC-tie list has neither pure mode but both as
    neighbours of its first three modes."""
    assert len(E.REFINE_ROTATION) == 7 and len(S.ALL_SIZES) == 70
    assert [E.refine_config(s) for s in S.ALL_SIZES] == [E.REFINE_ROTATION[i % 7] for i in range(70)]
    for modes, seeds in E.REFINE_ROTATION + (E.PDPC_TIE_CONFIG, E.OTHER_CONFIG):
        assert list(modes) == sorted(set(modes)) and 1 <= seeds <= RR.MAX_SEEDS and all(A.FIRST <= m <= A.LAST for m in modes)
    assert ((34,), 1) in E.REFINE_ROTATION and any(len(m) == s for m, s in E.REFINE_ROTATION)
    two = np.array([[2, 66]])
    assert ((2, 66), 2) in E.REFINE_ROTATION and list(np.nonzero(RR.candidates(two, (2, 66))[0])[0] + A.FIRST) == [3, 65]
    modes, seeds = E.PDPC_TIE_CONFIG
    assert 18 not in modes and 50 not in modes and seeds == 3
    assert list(np.nonzero(RR.candidates(np.array([modes[:3]]), modes)[0])[0] + A.FIRST) == [16, 18, 20, 48, 50]
    assert all(s in S.ALL_SIZES for s in E.PDPC_TIE_SIZES) and E.refine_config(E.OTHER_SIZE) == (RR.EVEN_MODES, 2)
    assert (("A", 15, CALLER_REFS_CASE[0]), CALLER_REFS_CASE[1]) in FILTER_CASES and CALLER_REFS_CASE[0][0] % 128


@lru_cache(maxsize=None)
def _condition_totals():
    total = dict.fromkeys(E.REFINE_CONDITIONS, 0)
    for w, h in S.ALL_SIZES:
        modes, seeds = E.refine_config((w, h))
        _, _, un, r = E.refine_sweep_case(w, h, "noise", None, modes, seeds)
        for key, n in E.refine_conditions(w, h, modes, seeds, r, un).items():
            total[key] += n
    return total


@slow
@pytest.mark.parametrize("name", E.REFINE_CONDITIONS)
def test_rotation_reaches_the_edge_conditions(name):
    """Over the 70 noise frames with their configurations, from the restatement alone: mode 18 or
    50 is a candidate of available first-column and first-row CUs; candidates win at CUs that reach
    past the right edge, in the first column and in the first row; available 64x64 CUs have the
    full 2 * seeds candidates and fewer; launches hold an available and an unavailable 64x64 CU;
    mode 2 or mode 66 is a candidate."""
    assert sorted(FLOORS) == sorted(E.REFINE_CONDITIONS)
    assert _condition_totals()[name] >= FLOORS[name], (name, _condition_totals())


@pytest.mark.parametrize("size", E.PDPC_TIE_SIZES, ids=S.size_id)
def test_pdpc_tie_configuration_runs_both_pure_modes_on_substituted_lines(size):
    """Every boundary of an available CU at (0, 0) is the 512 substitute, so all modes tie: seeds
    17, 19, 49, candidates 16, 18, 20, 48, 50, nine modes tried, mode 16 wins."""
    w, h = size
    modes, seeds = E.PDPC_TIE_CONFIG
    _, refs, un, r = E.refine_sweep_case(w, h, "noise", None, modes, seeds)
    x, y, _, _ = E.geometry(w, h)
    k = np.nonzero(~un & (x == 0) & (y == 0))[0]
    assert k.size >= 4
    for _, cus, top, left, corner in E.boundary_sets(refs, un, w, h):
        at = np.isin(cus, k)
        assert np.all(top[at] == 512) and np.all(left[at] == 512) and np.all(corner[at] == 512)
    assert np.all(r["seeds"][k] == (17, 19, 49))
    assert all(list(np.nonzero(c)[0] + A.FIRST) == [16, 18, 20, 48, 50] for c in r["cand"][k])
    assert np.all(r["tried"][k] == 9) and np.all(r["ang_mode"][k] == A.MODE_BASE + 16)
    assert np.all(r["cost"][k][:, np.array([16, 17, 18, 19, 20, 48, 49, 50, 51]) - A.FIRST] == r["ang_cost"][k, None])


def test_the_host_calls_cuts_fall_inside_their_calls():
    """Arithmetic only: the refined call's chunk is 191 frames of 200 (`tried` does not count), the
    candidate call's 146 (k = 3: MIP table + Planar / DC table + angular table = 1 833 200 bytes a
    frame); neither is a multiple of the period, so the second chunk starts between base frames.
    With k = 1 the chunk would be 186, a multiple of 3, which is why the test does not use it."""
    assert E.CUT_SIZE in S.ALL_SIZES and layout.num_ctus(*E.CUT_SIZE) == 1 and E.TABLE_BYTES == 268435456
    refined = E.table_cut_chunk(E.refine_cut_bytes())
    assert refined == 191 and refined < E.CUT_FRAMES and refined % E.CUT_PERIOD
    assert E.candidates_cut_bytes(E.CAND_K) == 97840 * 4 + 5380 * 2 * 4 + 5380 * 65 * 4 == 1833200
    cand = E.table_cut_chunk(E.candidates_cut_bytes(E.CAND_K))
    assert cand == 146 and cand < E.CUT_FRAMES and cand % E.CUT_PERIOD == 2
    assert E.table_cut_chunk(E.candidates_cut_bytes(1)) == 186 and 186 % E.CUT_PERIOD == 0 and E.CAND_K > 1


def test_the_cut_case_tells_its_base_frames_apart():
    """The three base frames differ in every output compared, and all three families win CUs."""
    _, un, fine, lists = E.cut_case()
    for a, b in ((0, 1), (1, 2), (0, 2)):
        for key in ("cost", "ang_mode", "ang_cost", "tried"):
            assert not np.array_equal(fine[a][key], fine[b][key]), (a, b, key)
        assert not np.array_equal(lists[a][0], lists[b][0]) and not np.array_equal(lists[a][1], lists[b][1])
    for modes, costs in lists:
        _assert_families(modes, costs, un)


def _assert_families(modes, costs, un):
    """From the reference alone: the 0xff / UNAVAILABLE pattern is the availability set, and MIP,
    Planar / DC and angular modes all win CUs."""
    assert np.array_equal(modes == 0xFF, np.broadcast_to(un[:, None], modes.shape))
    assert np.array_equal(costs == UN, np.broadcast_to(un[:, None], costs.shape))
    won = np.bincount(E.family_of(modes[~un, 0]), minlength=3)
    assert won.all(), won


@pytest.mark.parametrize("filt", CHAIN_FILTERS, ids=_filter_id)
@pytest.mark.parametrize("p", FIFTH, ids=_id)
def test_candidate_chain_inputs_mix_all_three_families(p, filt):
    """The 0xff / UNAVAILABLE pattern of every candidate case is its filter's availability set, and
    MIP, Planar / DC and angular modes all win CUs in it (a few seconds a case: the 65-mode table)."""
    w, h = p[2]
    _, un, modes, costs, _ = E.candidates_case(w, h, filt)
    assert np.array_equal(un, mipgpu.unavailable_cus(w, h, filt))
    _assert_families(modes, costs, un)


# ---------------------------------------------------------------- GPU: the kernel at every residue
def _decisions(want, un, salt):
    """Decisions to merge into, as tests/test_gpu_angular_refine.py test_multipass makes them: costs
    at and around the refined pair's own (ties included), about 5 % dead entries."""
    rng = np.random.default_rng(salt)
    near = np.where(want["ang_cost"] == UN, 0, want["ang_cost"]).astype(np.int64)
    cost = (near + rng.integers(-40, 41, near.shape) * rng.integers(0, 2, near.shape)).clip(0).astype(np.int32)
    mode = rng.integers(0, 12, cost.shape).astype(np.uint8)
    dead = un | (rng.random(cost.shape) < 0.05)
    cost[dead], mode[dead] = UN, 0xFF
    return mode, cost, dead


def _bad_cus(w, h, bad, g, t, first=A.FIRST):
    """The first few differing CUs with their place, shape and (got, want), for a table by mode
    (column + first)."""
    shape, x, y, _, _ = layout.cu_geometry(w, h, bad[:4])
    out = []
    for i, k in enumerate(bad[:4]):
        if g.ndim == 2:
            slots = np.nonzero(g[k] != t[k])[0][:6]
            diff = {int(s) + first: (int(g[k, s]), int(t[k, s])) for s in slots}
        else:
            diff = (int(g[k]), int(t[k]))
        out.append((int(k), "x=%d y=%d %s" % (x[i], y[i], layout.SHAPES[shape[i]].name), diff))
    return out


def _refine_and_check(eng, frame, un, modes, seeds, want, tag, refs=None, on=None):
    """One call with every output and a merge into prefilled decisions; everything against the
    restatement `want` and A.merge, on the CUs `on` (default: all); returns what the call gave."""
    w, h = frame.shape[1], frame.shape[0]
    on = np.ones(un.size, bool) if on is None else on
    best_mode, best_cost, dead = _decisions(want, un, 7 * w + h)
    arena = Arena(1, un.size)
    m, c = _dev(best_mode[None]), _dev(best_cost[None])
    assert eng.angular_refine_device(_dev(frame[None]), modes=modes, seeds=seeds, bias=MERGE_BIAS, best_mode=m, best_cost=c,
                                     refs=None if refs is None else _dev(refs[None]), **arena.outputs(ALL_OUT)) is None
    got, clean = arena.read(ALL_OUT)
    got = {key: v[0] for key, v in got.items()}
    got["best_mode"], got["best_cost"] = m.cpu().numpy()[0], c.cpu().numpy()[0]
    assert clean, tag
    want = dict(want)
    want["best_mode"], want["best_cost"] = (v[0] for v in A.merge(best_mode[None], best_cost[None], want["ang_mode"][None],
                                                                  want["ang_cost"][None], MERGE_BIAS))
    for key in ALL_OUT + ("best_mode", "best_cost"):
        g, t = got[key], want[key]
        bad = np.nonzero((g != t).reshape(un.size, -1).any(axis=1) & on)[0]
        assert bad.size == 0, (tag, key, bad.size, _bad_cus(w, h, bad, g, t))
    assert np.array_equal(want["best_mode"][dead], best_mode[dead]) and np.all(want["best_cost"][dead] == UN)
    if (~un).sum() > 100:                                     # the merge takes some CUs and leaves others
        taken = want["best_mode"] != best_mode
        assert taken.any() and (~taken & ~dead).any() and np.all(want["best_mode"][taken] >= A.MODE_BASE + A.FIRST)
    return got


def _assert_pattern(got, want, un, modes, tag):
    """Listed and candidate slots of available CUs are defined, everything else is UNAVAILABLE;
    tried == 0 and ang_mode == 0xff exactly on the unavailable CUs."""
    ev = want["evaluated"]
    assert np.array_equal(ev, (RR.listed_mask(modes)[None, :] | want["cand"]) & ~un[:, None])
    assert ev[~un].any(axis=1).all() and not want["cand"][un].any()
    for key in E.TABLES:
        assert np.all(got[key][ev] != UN) and np.all(got[key][~ev] == UN), (tag, key)
    assert np.array_equal(got["tried"] == 0, un) and np.array_equal(got["ang_mode"] == 0xFF, un), tag
    assert np.array_equal(got["ang_cost"] == UN, un) and np.array_equal(got["tried"], ev.sum(axis=1)), tag


@gpu
@pytest.mark.parametrize("p", SWEEP, ids=_id)
def test_refine_at_every_residue(gpu_available, p):
    """One noise frame, original references, the size's configuration: the three tables, the ang
    pair, `tried` and a merge into prefilled near-tie decisions in one call, the UNAVAILABLE
    pattern and the guards."""
    w, h = p[2]
    modes, seeds = E.refine_config((w, h))
    frame, _, un, want = E.refine_sweep_case(w, h, "noise", None, modes, seeds)
    assert np.array_equal(un, mipgpu.unavailable_cus(w, h)) and (~un).any()
    with MipEngine(w, h) as eng:
        got = _refine_and_check(eng, frame, un, modes, seeds, want, (w, h))
    _assert_pattern(got, want, un, modes, (w, h))


@gpu
@pytest.mark.parametrize("size", E.PDPC_TIE_SIZES, ids=S.size_id)
def test_refine_pdpc_candidates_on_substituted_lines(gpu_available, size):
    """(17, 19, 49, 51) with three seeds: at the CUs at (0, 0) modes 18 and 50 run as per-lane
    candidates on substituted boundaries; nine modes tried, mode 16 wins."""
    w, h = size
    modes, seeds = E.PDPC_TIE_CONFIG
    frame, _, un, want = E.refine_sweep_case(w, h, "noise", None, modes, seeds)
    x, y, _, _ = E.geometry(w, h)
    origin = ~un & (x == 0) & (y == 0)
    with MipEngine(w, h) as eng:
        got = _refine_and_check(eng, frame, un, modes, seeds, want, (w, h))
    _assert_pattern(got, want, un, modes, (w, h))
    assert origin.sum() >= 4 and np.all(got["tried"][origin] == 9) and np.all(got["ang_mode"][origin] == A.MODE_BASE + 16)


@gpu
@pytest.mark.parametrize("case", FILTER_CASES, ids=lambda c: _id(c[0]) + "-" + c[1][len("filterFrame_"):])
def test_refine_with_engine_filters(gpu_available, case):
    """`edges` frames, the engine filters the references itself, the configuration of the size's
    sweep index (even / 2 for the six filters at 136x72): against the restatement on the oracle's
    filtered frame with that filter's availability set."""
    (_, _, (w, h)), filt = case
    modes, seeds = E.refine_config((w, h))
    frame, refs, un, want = E.refine_sweep_case(w, h, "edges", filt, modes, seeds)
    assert np.array_equal(un, mipgpu.unavailable_cus(w, h, filt)) and (~un).any()
    if filt in S.SEP and w % 128:
        assert E.max_boundary_or_corner(refs, un, w, h) > 1023
    with MipEngine(w, h, filter=filt) as eng:
        got = _refine_and_check(eng, frame, un, modes, seeds, want, (w, h, filt))
    _assert_pattern(got, want, un, modes, (w, h, filt))


@gpu
def test_refine_with_caller_references_at_a_wrapped_size(gpu_available):
    """The oracle's filtered frame passed as d_refs gives what the engine-filtered call gives, on
    every CU available in both sets; the call's own set is the one of original references."""
    (w, h), filt = CALLER_REFS_CASE
    modes, seeds = E.refine_config((w, h))
    frame, refs, un_f, want = E.refine_sweep_case(w, h, "edges", filt, modes, seeds)
    un_o = mipgpu.unavailable_cus(w, h)
    both = ~un_f & ~un_o
    assert (both & E.wrapped(w, h)).any() and (un_f & ~un_o).any() and not np.array_equal(refs, frame)
    with MipEngine(w, h, filter=filt) as eng:
        engine = _refine_and_check(eng, frame, un_f, modes, seeds, want, (w, h, "engine"))
        caller = _refine_and_check(eng, frame, un_f, modes, seeds, want, (w, h, "caller"), refs=refs, on=both)
    for key in ALL_OUT:
        assert np.array_equal(caller[key][both], engine[key][both]), key
    assert np.array_equal(caller["tried"] == 0, un_o) and np.array_equal(caller["ang_mode"] == 0xFF, un_o)


# ---------------------------------------------------------------- GPU: the host calls across their cuts
def _cut_frames():
    base, un, fine, lists = E.cut_case()
    return base[np.arange(E.CUT_FRAMES) % E.CUT_PERIOD], un, fine, lists


@gpu
def test_refined_host_call_crosses_the_256_mib_cut(gpu_available):
    """200 frames of period 3 at 60x52 on max_batch = 200, even list, two seeds: with the table
    the chunk is 191 frames, then 9, so the second chunk starts at a frame index that is no
    multiple of the period; without the table the call is one chunk and gives the same pair and
    `tried`."""
    w, h = E.CUT_SIZE
    chunk = E.table_cut_chunk(E.refine_cut_bytes())
    assert chunk < E.CUT_FRAMES and chunk % E.CUT_PERIOD
    frames, un, fine, _ = _cut_frames()
    modes, seeds = E.CAND_ANGULAR
    with MipEngine(w, h, max_batch=E.CUT_FRAMES) as eng:
        host = eng.angular_refine(frames, modes=modes, seeds=seeds, table=True)
        pair = eng.angular_refine(frames, modes=modes, seeds=seeds)
    assert sorted(host) == ["ang_cost", "ang_mode", "cost", "tried"] and sorted(pair) == ["ang_cost", "ang_mode", "tried"]
    assert host["cost"].shape == (E.CUT_FRAMES, un.size, A.MODES)
    for f in range(E.CUT_FRAMES):                             # (frame by frame: no second copy of the table)
        want = fine[f % E.CUT_PERIOD]
        assert np.array_equal(host["cost"][f], want["cost"]), ("cost", f, chunk)
        for res, tag in ((host, "table"), (pair, "pair")):
            for key in ("ang_mode", "ang_cost", "tried"):
                assert np.array_equal(res[key][f], want[key]), (tag, key, f, chunk)


@gpu
def test_candidates_host_call_crosses_its_cut(gpu_available):
    """The same 200 frames through eng.candidates (k = 3, Planar / DC, even list with two seeds) on
    a default engine: 1 833 200 bytes of tables a frame make the chunk 146 frames, then 54, and
    146 % 3 == 2."""
    w, h = E.CUT_SIZE
    chunk = E.table_cut_chunk(E.candidates_cut_bytes(E.CAND_K))
    assert chunk < E.CUT_FRAMES and chunk % E.CUT_PERIOD
    frames, un, _, lists = _cut_frames()
    modes, seeds = E.CAND_ANGULAR
    with MipEngine(w, h, max_batch=E.CUT_FRAMES) as eng:
        got = eng.candidates(frames, k=E.CAND_K, angular=modes, seeds=seeds, intra_bias=E.CAND_INTRA_BIAS,
                             angular_bias=E.CAND_ANGULAR_BIAS)
    assert sorted(got) == ["costs", "modes"] and got["modes"].shape == (E.CUT_FRAMES, un.size, E.CAND_K)
    for f in range(E.CUT_FRAMES):
        want = lists[f % E.CUT_PERIOD]
        assert np.array_equal(got["modes"][f], want[0]) and np.array_equal(got["costs"][f], want[1]), (f, chunk)


# ---------------------------------------------------------------- GPU: the candidate chain at every fifth size
@gpu
@pytest.mark.parametrize("filt", CHAIN_FILTERS, ids=_filter_id)
@pytest.mark.parametrize("p", FIFTH, ids=_id)
def test_candidate_chain_at_every_fifth_size(gpu_available, p, filt):
    """eng.candidates on the `edges` frame (k = 3, Planar / DC, refined angular stage: even list,
    two seeds), original references and the engine's own filters: lists and costs against
    tests/candidates_ref.py over the oracle's search, tests/intra_ref.py and the refined table;
    0xff / UNAVAILABLE exactly on the filter's unavailable set."""
    w, h = p[2]
    frame, un, modes, costs, _ = E.candidates_case(w, h, filt)
    _assert_families(modes, costs, un)
    with MipEngine(w, h, filter=filt) as eng:
        got = eng.candidates(frame[None], k=E.CAND_K, angular=E.CAND_ANGULAR[0], seeds=E.CAND_ANGULAR[1], intra_bias=E.CAND_INTRA_BIAS,
                             angular_bias=E.CAND_ANGULAR_BIAS)
    for key, want in (("modes", modes), ("costs", costs)):
        g = got[key][0]
        bad = np.nonzero((g != want).any(axis=1))[0]
        assert bad.size == 0, ((w, h, filt), key, bad.size, _bad_cus(w, h, bad, g, want, 0))     # (by list entry)
    assert np.array_equal(got["modes"][0] == 0xFF, np.broadcast_to(un[:, None], modes.shape))
    assert np.array_equal(got["costs"][0] == UN, np.broadcast_to(un[:, None], costs.shape))
