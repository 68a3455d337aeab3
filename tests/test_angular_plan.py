"""Angular intra costs on the CPU (no GPU): the host walk of csrc/angular_plan.h -- the
per-4x4-block arithmetic the kernel runs one lane per block, the argmin over the mode list and
the merge -- compiled stand-alone (tests/cpp/test_angular_plan.cpp, with
-fsanitize=address,undefined; no preloaded library) equals the numpy restatement
tests/angular_ref.py bit for bit in every table, in the best angular mode and in the merge, on
structured, noise and 0 / 1023 frames at 136x72 for all 65 modes, and on the residue sweep's
frames and mode list (tests/edge_sweep_cases.py) at every fifth sweep size, where the exactly
frame-sized arrays turn a read past the frame's end into a sanitizer report; the same program checks the
argument rules (bad mode lists, a bias out of range), and lists the CUs whose corner sample an
engine filter leaves undefined, which pins the availability set."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import angular_cases as AC
import angular_ref as A
import edge_sweep_cases as E
import mipgpu
import size_sweep
from mipgpu import layout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER = AC.FILTER
UN = layout.UNAVAILABLE

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("angular_plan") / "test_angular_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "vvc-mip-gpu_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", str(exe),
                           os.path.join(REPO, "tests", "cpp", "test_angular_plan.cpp")])
    return str(exe)


def run_plan(exe, tmp_path, frames, refs, unavailable, modes, best_mode, best_cost, bias):
    nf, h, w = frames.shape
    ncu = unavailable.size
    modes = () if modes is None else modes
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([w, h, nf, bias, len(modes)], np.int32).tobytes())
        for a, dt in ((modes, np.uint8), (frames, np.uint16), (refs, np.uint16), (unavailable, np.uint8), (best_mode, np.uint8),
                      (best_cost, np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    r = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "angular_plan: ok" in r.stdout, (r.returncode, r.stdout + r.stderr)
    raw = open(dst, "rb").read()
    out, at = {}, 0
    table = (np.int32, nf * ncu * 65, (nf, ncu, 65))
    for key, (dt, count, shape) in (("cost", table), ("sad", table), ("satd", table), ("ang_mode", (np.uint8, nf * ncu, (nf, ncu))),
                                    ("ang_cost", (np.int32, nf * ncu, (nf, ncu))), ("best_mode", (np.uint8, nf * ncu, (nf, ncu))),
                                    ("best_cost", (np.int32, nf * ncu, (nf, ncu)))):
        out[key] = np.frombuffer(raw, dt, count, at).reshape(shape)
        at += count * np.dtype(dt).itemsize
    assert at == len(raw)
    return out


def _decisions(ref, un, seed):
    """Decisions for the merge: around the best angular costs, with exact ties and unavailable CUs."""
    rng = np.random.default_rng(seed)
    near = np.where(ref["ang_cost"] == UN, 0, ref["ang_cost"])
    best_cost = (near + rng.integers(-40, 41, near.shape) * rng.integers(0, 2, near.shape)).clip(0).astype(np.int32)
    best_mode = rng.choice(np.array([0, 3, 11, 0xF0, 0xF1], np.uint8), best_cost.shape)
    dead = np.broadcast_to(un, best_cost.shape) | (rng.random(best_cost.shape) < 0.05)
    best_cost[dead], best_mode[dead] = UN, 0xFF
    return best_mode, best_cost, dead


@pytest.mark.parametrize("filt", (None, FILTER), ids=("orig", "1d_int"))
def test_host_walk_equals_the_restatement(plan_exe, tmp_path, filt):
    """All 65 modes at 136x72; the program itself refuses bad lists and a bias out of range, and
    checks the per-sample predictor against the per-block step."""
    w, h = 136, 72
    frames, refs, un, ref = AC.case(w, h, filt)
    assert un.any() and not un.all()
    if filt is not None:
        assert refs.max() > 1023                              # the only way the clip can fire
    best_mode, best_cost, dead = _decisions(ref, un, w)
    for bias, n in ((7, 3), (0, 1)):                          # (the second bias on one frame: the walk is the same)
        got = run_plan(plan_exe, tmp_path, frames[:n], refs[:n], un, None, best_mode[:n], best_cost[:n], bias)
        for key in AC.TABLES + ("ang_mode", "ang_cost"):
            assert np.array_equal(got[key], ref[key][:n]), key
        assert np.array_equal(got["cost"][:, :, 0] == UN, np.broadcast_to(un, best_cost[:n].shape))
        mode, cost = A.merge(best_mode[:n], best_cost[:n], ref["ang_mode"][:n], ref["ang_cost"][:n], bias)
        assert np.array_equal(got["best_mode"], mode) and np.array_equal(got["best_cost"], cost)
        assert (mode >= 0x82).any() and (mode < 12).any() and (mode == 0xF0).any()
        assert np.array_equal(mode[dead[:n]], best_mode[:n][dead[:n]])    # unavailable CUs stay as they are
        ties = (best_cost[:n] == ref["ang_cost"][:n].astype(np.int64) + bias) & ~dead[:n]
        assert ties.any() and np.array_equal(mode[ties], best_mode[:n][ties])


def test_host_walk_with_a_mode_list(plan_exe, tmp_path):
    """One frame, a list spanning both classes and both angle signs: unlisted slots are
    UNAVAILABLE, listed ones the all-modes values, the best is taken over the list only."""
    w, h, modes = 136, 72, (2, 18, 27, 34, 45, 50, 66)
    frames, refs, un, full = AC.case(w, h, None)
    best_mode, best_cost, _ = _decisions(full, un, 5)
    got = run_plan(plan_exe, tmp_path, frames[:1], refs[:1], un, modes, best_mode[:1], best_cost[:1], 3)
    slots = np.array(modes) - 2
    listed = np.zeros(65, bool)
    listed[slots] = True
    for key in AC.TABLES:
        assert np.array_equal(got[key][..., listed], full[key][:1][..., listed]), key
        assert np.all(got[key][..., ~listed] == UN), key
    am, ac = A.best(got["cost"])
    assert np.array_equal(got["ang_mode"], am) and np.array_equal(got["ang_cost"], ac)
    assert set(np.unique(am)) <= {0x80 + m for m in modes} | {0xFF}
    mode, cost = A.merge(best_mode[:1], best_cost[:1], am, ac, 3)
    assert np.array_equal(got["best_mode"], mode) and np.array_equal(got["best_cost"], cost)


def _walk_equals(plan_exe, tmp_path, case, w, h, bias):
    """One frame of an edge_sweep_cases.angular_sweep_case through the stand-alone program
    (exactly frame-sized arrays: a read past the frame's end by an available CU is an
    AddressSanitizer report): tables, pair and merge equal the restatement."""
    frame, refs, un, tabs = case
    ref = {k: v[None] for k, v in tabs.items()}
    best_mode, best_cost, dead = _decisions(ref, un, w + h)
    got = run_plan(plan_exe, tmp_path, frame[None], refs[None], un, E.SWEEP_MODES, best_mode, best_cost, bias)
    for key in AC.TABLES + ("ang_mode", "ang_cost"):
        bad = np.nonzero((got[key][0] != tabs[key]).reshape(un.size, -1).any(axis=1))[0]
        assert bad.size == 0, ((w, h), key, bad.size, bad[:4], got[key][0][bad[:4]], tabs[key][bad[:4]])
    assert np.array_equal(got["cost"][0, :, E.SWEEP_MODES[0] - 2] == UN, un)
    mode, cost = A.merge(best_mode, best_cost, ref["ang_mode"], ref["ang_cost"], bias)
    assert np.array_equal(got["best_mode"], mode) and np.array_equal(got["best_cost"], cost)
    assert np.array_equal(mode[dead], best_mode[dead])
    return mode


@pytest.mark.parametrize("size", E.FIFTH, ids=size_sweep.size_id)
def test_host_walk_at_every_fifth_sweep_size(plan_exe, tmp_path, size):
    """The residue sweep's noise frames and mode list (tests/edge_sweep_cases.py), original
    references: partial CTUs on both axes, windows that wrap over several frame rows."""
    w, h = size
    mode = _walk_equals(plan_exe, tmp_path, E.angular_sweep_case(w, h), w, h, 7)
    assert (mode >= 0x82).any() and (mode < 12).any()


def test_host_walk_on_a_filtered_edges_frame(plan_exe, tmp_path):
    """An `edges` frame through the oracle's separable filter at W % 128 != 0: references above
    1023 on available CUs, that filter's availability set."""
    w, h = 152, 176
    assert (w, h) in E.FIFTH and w % 128
    case = E.angular_sweep_case(w, h, "edges", E.FILTER_SEP)
    assert E.max_boundary_or_corner(case[1], case[2], w, h) > 1023
    assert (case[2] & ~mipgpu.unavailable_cus(w, h)).any()     # the filter takes CUs away
    _walk_equals(plan_exe, tmp_path, case, w, h, 0)


def test_no_available_cu_has_an_undefined_corner(plan_exe):
    """The availability set is unchanged by the corner sample: for the 70 sizes of the size sweep
    and the eight filters, every CU whose corner sample (x > 0, y > 0) lies in the filter's
    undefined set (work_plan.h filter_poison) is already in mipgpu.unavailable_cus."""
    sizes = [tuple(s) for s in size_sweep.ALL_SIZES]
    assert len(sizes) == 70
    args = [str(v) for wh in sizes for v in wh]
    r = subprocess.run([plan_exe, "corner"] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("corners: ok\n"), (r.returncode, r.stdout[-400:] + r.stderr)
    hits = {}
    for line in r.stdout.splitlines()[:-1]:
        w, h, filt, cu = (int(v) for v in line.split())
        hits.setdefault((w, h, filt), []).append(cu)
    assert hits and {f for _, _, f in hits} == set(range(8))    # every filter leaves corners undefined somewhere
    for (w, h, filt), cus in hits.items():
        assert (w, h) in sizes
        un = mipgpu.unavailable_cus(w, h, mipgpu.FILTERS[filt])
        assert un[np.array(cus)].all(), (w, h, filt, [c for c in cus if not un[c]][:5])
