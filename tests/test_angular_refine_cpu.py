"""Coarse-to-fine angular search on the CPU (no GPU): the numpy restatement
tests/angular_refine_ref.py pinned by hand-checkable cases (frames one pure or diagonal mode
predicts exactly reached through a neighbour, ties on a uniform frame, seeds at the ends of the
mode range, shared neighbours, the lists (2, 34, 66), one mode and all 65); the host walk
angular_refine_frames_host of csrc/angular_plan.h, compiled stand-alone with
-fsanitize=address,undefined (tests/cpp/test_angular_refine.cpp, exactly frame-sized arrays),
against the restatement bit for bit; the candidate step exhaustively and the argument rules in
that program; the header's and the binding's constants and signatures; the launcher's grid cap
and the kernel's resources in the built library."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import angular_cases as AC
import angular_ref as A
import angular_refine_ref as RR
import edge_sweep_cases as E
import kernel_resources
import launch_caps
import mipgpu
import size_sweep
from mipgpu import layout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UN = layout.UNAVAILABLE
LISTS = {"even": RR.EVEN_MODES, "odd": RR.ODD_MODES, "sparse": RR.SPARSE_MODES}
JOBS = [(name, seeds) for name in LISTS for seeds in (1, 2, 3)]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


# ---------------------------------------------------------------- hand-checkable cases
def _inner(w, h, kind):
    un = mipgpu.unavailable_cus(w, h)
    _, x, y, bw, _ = layout.cu_geometry(w, h, np.arange(un.size))
    inner = ~un & (x > 0) & (y > 0)
    if kind != "x":
        inner &= x + bw <= w                                  # (tests/test_angular_cpu.py says why)
    return un, inner


@pytest.mark.parametrize("kind, mode", (("x", 50), ("y", 18), ("x-y", 34)))
def test_structured_frames_reach_their_mode_through_a_neighbour(kind, mode):
    """The odd list 3..65 does not hold 18, 34 or 50; with one seed the best odd mode is a
    neighbour of the exact mode, which then is a candidate and wins at cost 0.  That is every
    interior CU of f(x - y); of f(x) and f(y), 5 of 4928 and 6 of 2569 CUs (4x32 / 8x32 and their
    transposes, where the random table happens to favour a far mode) rank another odd mode first
    and never see the exact one: the local minimum a coarse-to-fine search can end in.  Those are
    counted and held below 1 %; everywhere else the case is the hand-checkable one."""
    w, h = 136, 72
    frame = AC.structured(kind, w, h)
    un, inner = _inner(w, h, kind)
    full = A.tables(frame, frame, un)
    got = RR.refine(full, RR.ODD_MODES, 1)
    assert inner.sum() > 1000
    near = inner & np.isin(got["seeds"][:, 0], (mode - 1, mode + 1))
    trapped = inner & ~near
    assert trapped.sum() * 100 < inner.sum() and (kind != "x-y" or not trapped.any())
    assert np.all(got["cand"][near, mode - 2]) and np.all(got["ang_mode"][near] == 0x80 + mode) and not got["ang_cost"][near].any()
    assert not got["cand"][trapped, mode - 2].any() and np.all(got["ang_cost"][trapped] > 0)
    assert np.all(got["tried"][inner] == 34) and np.all(got["tried"][un] == 0)
    coarse_mode, coarse_cost = A.best(np.where(RR.listed_mask(RR.ODD_MODES), full["cost"], UN))
    assert np.all(coarse_cost[inner] > 0) and np.all(coarse_mode[inner] != 0x80 + mode)


def test_uniform_frame_ties():
    """Everything ties: with the even list and three seeds the seeds are 2, 4, 6, the candidates
    3, 5, 7, the result mode 2, and 36 modes are evaluated."""
    w, h = 136, 72
    frame = np.full((h, w), 700, np.uint16)
    un = mipgpu.unavailable_cus(w, h)
    got = RR.refine(A.tables(frame, frame, un), RR.EVEN_MODES, 3)
    ok = ~un
    assert np.all(got["seeds"][ok] == (2, 4, 6))
    want = np.zeros(65, bool)
    want[[1, 3, 5]] = True
    assert np.all(got["cand"][ok] == want) and not got["cand"][un].any()
    assert np.all(got["ang_mode"][ok] == 0x82) and np.all(got["tried"][ok] == 36) and np.all(got["tried"][un] == 0)
    assert np.all(got["ang_mode"][un] == 0xFF) and np.all(got["ang_cost"][un] == UN)


def _table(rows):
    """65-mode tables whose cost rows are given as {mode: cost} over a floor of 1000 + mode."""
    cost = np.tile(1000 + np.arange(2, 67), (len(rows), 1)).astype(np.int32)
    for r, row in enumerate(rows):
        for m, c in row.items():
            cost[r, m - 2] = c
    return {"cost": cost, "sad": cost + 1, "satd": cost * 2}


def test_seeds_at_the_ends_and_shared_neighbours():
    tabs = _table([{2: 5}, {66: 5}, {10: 5, 12: 6, 11: 1}, {10: 5, 12: 5, 14: 5}, {20: 7, 22: 7, 21: 7}, {20: 7, 22: 7, 19: 7}])
    one = RR.refine(tabs, RR.EVEN_MODES, 1)
    assert [np.nonzero(c)[0].tolist() for c in one["cand"][:2]] == [[1], [63]]          # modes 3 and 65: one candidate, no wrap
    assert one["tried"][:2].tolist() == [34, 34] and one["ang_mode"][:2].tolist() == [0x82, 0xC2]
    two = RR.refine(tabs, RR.EVEN_MODES, 2)
    assert two["seeds"][2].tolist() == [10, 12] and np.nonzero(two["cand"][2])[0].tolist() == [7, 9, 11]   # 9, 11, 13: 11 once
    assert two["tried"][2] == 36 and two["ang_mode"][2] == 0x80 + 11 and two["ang_cost"][2] == 1
    three = RR.refine(tabs, RR.EVEN_MODES, 3)
    assert three["seeds"][3].tolist() == [10, 12, 14] and np.nonzero(three["cand"][3])[0].tolist() == [7, 9, 11, 13]
    assert three["tried"][3] == 37 and three["ang_mode"][3] == 0x80 + 10               # ties: the lower mode
    # a candidate that ties the list's best: the lower mode number wins, candidate or not
    assert two["ang_mode"][4] == 0x80 + 20 and two["ang_mode"][5] == 0x80 + 19
    # a neighbour that is in the list is not a candidate and is not counted again
    assert not (three["cand"] & RR.listed_mask(RR.EVEN_MODES)).any()
    dense = RR.refine(tabs, (9, 10, 11, 40), 2)
    assert dense["seeds"][2].tolist() == [11, 10] and np.nonzero(dense["cand"][2])[0].tolist() == [10] and dense["tried"][2] == 5


def test_edge_list_one_mode_list_and_full_list():
    w, h = 136, 72
    _, _, un, full = AC.case(w, h, None)
    tabs = {k: full[k][1] for k in AC.TABLES}
    edge = RR.refine(tabs, RR.EDGE_MODES, 3)
    want = np.zeros(65, bool)
    want[[1, 31, 33, 63]] = True                              # 3, 33, 35, 65
    assert np.all(edge["cand"][~un] == want) and np.all(edge["tried"][~un] == 7)
    low = RR.refine(tabs, RR.EDGE_MODES, 1)
    assert set(np.unique(low["tried"][~un])) == {4, 5}        # a seed at 2 or 66 has one neighbour, the seed 34 two
    single = RR.refine(tabs, (40,), 3)
    assert np.all(single["seeds"][~un] == (40,)) and np.all(single["tried"][~un] == 3)
    assert np.array_equal(single["cost"][~un][:, [37, 38, 39]], tabs["cost"][~un][:, [37, 38, 39]])
    for seeds in (1, 2, 3):
        all65 = RR.refine(tabs, None, seeds)
        assert not all65["cand"].any() and np.all(all65["tried"][~un] == 65)
        for key in AC.TABLES:
            assert np.array_equal(all65[key], tabs[key]), key
        assert np.array_equal(all65["ang_mode"], full["ang_mode"][1]) and np.array_equal(all65["ang_cost"], full["ang_cost"][1])
    # never above the list's best, never below the 65-mode best
    for name, modes in LISTS.items():
        coarse = A.best(np.where(RR.listed_mask(modes), tabs["cost"], UN))[1]
        for seeds in (1, 2, 3):
            fine = RR.refine(tabs, modes, seeds)["ang_cost"]
            assert np.all(fine <= coarse) and np.all(fine >= full["ang_cost"][1]), (name, seeds)
            assert (fine < coarse).any()


# ---------------------------------------------------------------- the host walk
@pytest.fixture(scope="module")
def refine_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("angular_refine") / "test_angular_refine"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "vvc-mip-gpu_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", str(exe),
                           os.path.join(REPO, "tests", "cpp", "test_angular_refine.cpp")])
    return str(exe)


def run_refine(exe, tmp_path, frames, refs, unavailable, jobs, best_mode, best_cost, bias):
    """The program's outputs, one dict per (modes, seeds) job."""
    nf, h, w = frames.shape
    ncu = unavailable.size
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([w, h, nf, bias, len(jobs)], np.int32).tobytes())
        for a, dt in ((frames, np.uint16), (refs, np.uint16), (unavailable, np.uint8), (best_mode, np.uint8), (best_cost, np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
        for modes, seeds in jobs:
            modes = () if modes is None else modes
            f.write(np.array([seeds, len(modes)], np.int32).tobytes())
            f.write(np.array(modes, np.uint8).tobytes())
    r = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "angular_refine: ok" in r.stdout, (r.returncode, r.stdout + r.stderr)
    raw = open(dst, "rb").read()
    table = (np.int32, nf * ncu * 65, (nf, ncu, 65))
    per_cu = lambda dt: (dt, nf * ncu, (nf, ncu))
    outs, at = [], 0
    for _ in jobs:
        out = {}
        for key, (dt, count, shape) in (("cost", table), ("sad", table), ("satd", table), ("ang_mode", per_cu(np.uint8)),
                                        ("ang_cost", per_cu(np.int32)), ("tried", per_cu(np.uint8)), ("best_mode", per_cu(np.uint8)),
                                        ("best_cost", per_cu(np.int32))):
            out[key] = np.frombuffer(raw, dt, count, at).reshape(shape)
            at += count * np.dtype(dt).itemsize
        outs.append(out)
    assert at == len(raw)
    return outs


def _decisions(ang_cost, un, seed):
    """Decisions for the merge: around the given angular costs, with exact ties and unavailable CUs."""
    rng = np.random.default_rng(seed)
    near = np.where(ang_cost == UN, 0, ang_cost)
    best_cost = (near + rng.integers(-40, 41, near.shape) * rng.integers(0, 2, near.shape)).clip(0).astype(np.int32)
    best_mode = rng.choice(np.array([0, 3, 11, 0xF0, 0xF1], np.uint8), best_cost.shape)
    dead = np.broadcast_to(un, best_cost.shape) | (rng.random(best_cost.shape) < 0.05)
    best_cost[dead], best_mode[dead] = UN, 0xFF
    return best_mode, best_cost


def _walk_equals(exe, tmp_path, frames, refs, un, full, bias):
    """Every (list, seeds) job of JOBS on frames [n, H, W] with 65-mode tables `full`."""
    best_mode, best_cost = _decisions(full["ang_cost"], un, frames.shape[-1])
    got = run_refine(exe, tmp_path, frames, refs, un, [(LISTS[name], seeds) for name, seeds in JOBS], best_mode, best_cost, bias)
    for (name, seeds), out in zip(JOBS, got):
        want = RR.refine(full, LISTS[name], seeds)
        for key in RR.TABLES + ("ang_mode", "ang_cost", "tried"):
            assert np.array_equal(out[key], want[key]), (name, seeds, key)
        mode, cost = A.merge(best_mode, best_cost, want["ang_mode"], want["ang_cost"], bias)
        assert np.array_equal(out["best_mode"], mode) and np.array_equal(out["best_cost"], cost), (name, seeds)
        assert np.array_equal(mode[best_cost == UN], best_mode[best_cost == UN])


@needs_gxx
@pytest.mark.parametrize("size", ((136, 72), (60, 36)), ids=size_sweep.size_id)
def test_host_walk_equals_the_restatement(refine_exe, tmp_path, size):
    w, h = size
    frames, refs, un, full = AC.case(w, h, None)
    _walk_equals(refine_exe, tmp_path, frames, refs, un, full, 7)


@needs_gxx
@pytest.mark.parametrize("size", E.FIFTH, ids=size_sweep.size_id)
def test_host_walk_at_every_fifth_sweep_size(refine_exe, tmp_path, size):
    w, h = size
    frame, refs, un, tabs = E.angular_sweep_case(w, h, modes=None)
    _walk_equals(refine_exe, tmp_path, frame[None], refs[None], un, {k: v[None] for k, v in tabs.items()}, 0)


@needs_gxx
def test_candidate_step_top_list_and_argument_rules(refine_exe):
    """The program's own checks: the candidate step against a plain set computation for every
    seed tuple of up to three modes and five list masks, the running top three against a stable
    sort on lists full of ties, and the walk's argument rules (seeds 0 and 4, a bad list, a bad
    bias, no output, half a pair; `tried` alone is an output)."""
    r = subprocess.run([refine_exe, "rules"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "angular_refine rules: ok" in r.stdout, (r.returncode, r.stdout + r.stderr)


# ---------------------------------------------------------------- contract, binding, launcher, resources
def _header():
    with open(os.path.join(REPO, "include", "mipgpu.h")) as f:
        return f.read()


def test_header_and_python_constants_and_signatures():
    src = _header()
    assert re.search(r"#define MIP_ANGULAR_MAX_SEEDS 3\b", src) and mipgpu.ANGULAR_MAX_SEEDS == RR.MAX_SEEDS == 3
    assert mipgpu.ANGULAR_EVEN_MODES == RR.EVEN_MODES == AC.EVEN_MODES and len(mipgpu.ANGULAR_EVEN_MODES) == 33
    assert "ANGULAR_EVEN_MODES" in mipgpu.__all__ and "ANGULAR_MAX_SEEDS" in mipgpu.__all__
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    dev = re.search(r"int mip_angular_refine_device\((.*?)\);", code, re.S).group(1)
    assert [p.split()[-1].lstrip("*") for p in dev.split(",")] == [
        "e", "d_frames", "d_refs", "nframes", "modes", "nmodes", "seeds", "d_cost", "d_sad", "d_satd", "d_ang_mode", "d_ang_cost",
        "d_ang_tried", "bias", "d_best_mode", "d_best_cost", "stream"]
    host = re.search(r"int mip_angular_refine_frames\((.*?)\);", code, re.S).group(1)
    assert [p.split()[-1].lstrip("*") for p in host.split(",")] == [
        "e", "frames", "refs_or_null", "nframes", "modes", "nmodes", "seeds", "cost_out", "ang_mode_out", "ang_cost_out", "tried_out"]
    lib = mipgpu.library()
    assert len(lib.mip_angular_refine_device.argtypes) == 17 and len(lib.mip_angular_refine_frames.argtypes) == 11
    assert lib.mip_angular_refine_device.argtypes[6] is ctypes.c_int and lib.mip_angular_refine_device.argtypes[13] is ctypes.c_int32
    assert lib.mip_abi_version() == 7
    assert list(inspect.signature(mipgpu.MipEngine.angular_refine).parameters) == ["self", "frames", "refs", "modes", "seeds", "table"]
    assert list(inspect.signature(mipgpu.MipEngine.angular_refine_device).parameters) == [
        "self", "frames", "modes", "seeds", "cost", "sad", "satd", "ang_mode", "ang_cost", "tried", "refs", "bias", "best_mode", "best_cost",
        "stream"]
    sig = inspect.signature(mipgpu.MipEngine.angular_refine_device).parameters
    assert sig["seeds"].default == 1 and sig["bias"].default == 0 and inspect.signature(mipgpu.MipEngine.angular_refine).parameters["seeds"].default == 1


def test_entry_points_refuse_a_null_engine():
    lib = mipgpu.library()
    out = (ctypes.c_uint8 * 8)()
    assert lib.mip_angular_refine_device(None, None, None, 1, None, 0, 1, None, None, None, None, None, out, 0, None, None, None) != 0
    assert b"engine is NULL" in lib.mip_last_error()
    assert lib.mip_angular_refine_frames(None, None, None, 1, None, 0, 1, None, None, None, out) != 0
    assert b"engine is NULL" in lib.mip_last_error()


def test_launch_cap_is_the_angular_launcher_s():
    """launch_angular_refine: angular_kernel's items and grid cap (tests/angular_cases.angular_cap
    sizes the multi-pass GPU test), and angular_kernel's item walk: all six launchers and the code
    all six cost kernels run -- the one body four of them wrap, the own bodies of the other two -- go
    through the one grid rule and item walk of launch_caps.WINDOW_HEADER, and no angular file has a
    cap or an item count of its own."""
    for launcher, kernel in AC.COST_KERNELS:
        assert launch_caps.uses_window_rules(AC.COST_SOURCE, launcher, kernel), launcher
        # nothing but a call of the shared body -- or, for the two measured slower that way, no wrapper at all
        assert launch_caps.wrapped_body(AC.COST_SOURCE, kernel) == (None if kernel in AC.COST_OWN_BODY else AC.COST_BODY), kernel
    body = launch_caps.launcher_body(launch_caps.WINDOW_HEADER, "launch_window_kernel")
    caps = launch_caps.CAP_EXPRESSION.findall(body)
    assert caps == [(str(AC.ANGULAR_ITEMS_PER_CU),) * 2], caps
    assert "a.nframes * a.nctus * kItemsPerCtu" in body
    sources = sorted(f for f in os.listdir(launch_caps.CSRC) if f.startswith("mip_angular"))
    assert sources == ["mip_angular.hip", "mip_angular_dev.h"]
    walks = 0
    for source in sources:
        with open(launch_caps.CSRC + "/" + source) as f:
            own = f.read()
        assert not launch_caps.CAP_EXPRESSION.findall(own) and "kItemsPerCtu =" not in own and "big = k <" not in own, source
        walks += own.count("g += gridDim.x")
    assert walks == 1 + len(AC.COST_OWN_BODY)                               # the item loop: the shared body's, and the two own bodies'
    kernel = launch_caps.kernel_body(AC.COST_SOURCE, "angular_refine_kernel")
    assert kernel.startswith("void %s(" % AC.COST_BODY)
    text = launch_caps.window_text()
    assert "g += gridDim.x" in kernel and text.count("const bool big = k < %d;" % AC.ANGULAR_BIG_ITEMS) == 1
    assert text.count("constexpr int kItemsPerCtu = 4 + kIntraBlocks;") == 1


def _kernel(name):
    found = [v for k, v in kernel_resources.kernels(mipgpu.LIB_PATH).items() if re.search(r"\d+%sE" % name, k)]
    assert len(found) == 1, name
    return found[0]


def test_kernel_resources():
    """angular_refine_kernel: no scratch, no spilled vector register, at most 168 VGPRs -- 512 per
    SIMD lane over three waves, in the allocation unit of 8 -- so three waves per SIMD like
    angular_kernel; both with exactly the LDS of their layouts.  The VGPR figures themselves are
    pinned in tests/test_kernel_resources.py."""
    mipgpu.library()
    for name, lds in (("angular_refine_kernel", 13612), ("angular_kernel", 13308)):
        k = _kernel(name)
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, name
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 512 // 3 // 8 * 8 == 168, name
        assert k[".group_segment_fixed_size"] == lds and 3 * lds <= 160 * 1024, name


def test_gpu_case_set_is_not_vacuous():
    """The coverage conditions of tests/test_gpu_angular_refine.py's case set, on the restatement
    alone: candidates of negative and of positive angle in both classes, a single candidate at a
    seed of 2 or 66, a shared neighbour, candidates and list modes both among the winners, and a
    32x32 block with eight or more distinct candidate sets among the CUs of one shape."""
    import angular_refine_cases as RC
    seen = RC.coverage()
    assert all(seen.values()), seen
