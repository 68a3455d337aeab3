"""VVC's 4-tap angular interpolation on the CPU (no GPU): the numpy restatement
tests/angular_tap4_ref.py pinned by hand-checkable cases (a constant line, an impulse line that
exposes every coefficient of both tables with its sign, the two equality consequences of the
contract, a line that drives a cubic sum below 0 and above 1023, and mip_angular_filter against the
thresholds spelled out); the C++ host walks of csrc/angular_plan.h, compiled stand-alone with
-fsanitize=address,undefined (tests/cpp/test_angular_tap4.cpp), against the restatement bit for bit
under both reference settings; the header's and the binding's constants, the switch's argument
rules and the pinned signatures; the new kernels' resources in the built library; and the coverage
conditions of the GPU cases."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import angular_ext_cases as XC
import angular_ext_ref as X
import angular_ref as A
import angular_refine_ref as RR
import angular_tap4_cases as TC
import angular_tap4_ref as T
import kernel_resources
import mipgpu
import size_sweep
from mipgpu import layout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UN = layout.UNAVAILABLE
W, H = TC.SIZE

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _geometry(w, h):
    _, x, y, bw, bh = layout.cu_geometry(w, h, np.arange(layout.num_ctus(w, h) * layout.CUS_PER_CTU))
    return x, y, bw, bh


# ---------------------------------------------------------------- hand-checkable cases
def test_tables_as_the_header_writes_them():
    """Every row of both tables sums to 64, fC[0] is the identity, fG[0] is [1 2 1] / 4 in 64ths,
    fC[32 - f] is fC[f] reversed, and a few rows by hand."""
    assert T.FC.shape == T.FG.shape == (32, 4) and np.all(T.FC.sum(axis=1) == 64) and np.all(T.FG.sum(axis=1) == 64)
    assert T.FC[0].tolist() == [0, 64, 0, 0] and T.FG[0].tolist() == [16, 32, 16, 0]
    assert T.FC[16].tolist() == [-4, 36, 36, -4] and T.FC[3].tolist() == [-2, 60, 7, -1] and T.FC[13].tolist() == [-5, 44, 29, -4]
    assert T.FC[29].tolist() == [-1, 7, 60, -2] and T.FC[31].tolist() == [0, 2, 63, -1]
    assert T.FG[31].tolist() == [1, 17, 31, 15] and T.FG[16].tolist() == [8, 24, 24, 8]
    for f in range(1, 32):
        assert T.FC[32 - f].tolist() == T.FC[f][::-1].tolist(), f
    assert T.FC.min() == -6 and (T.FC < 0).sum() == 58 and T.FG.min() == 0


def _lines(w, h, v):
    """Lines of angular_ext_ref.boundaries' shape for one CU, constant v."""
    return np.full((1, w + h), v, np.int64), np.full((1, h + w), v, np.int64), np.array([v], np.int64)


@pytest.mark.parametrize("w, h", ((4, 4), (8, 4), (8, 8), (16, 32), (64, 64)))
def test_a_constant_line_predicts_the_constant_in_every_mode(w, h):
    for v in (0, 1, 511, 1023):
        top, left, corner = _lines(w, h, v)
        assert np.all(T.predict(top, left, corner, w, h) == v), v


# (w, h) by which table mode 51 / 49 / 17 / 19 (distance 1 from a pure mode) takes: 8x32 is size
# class (3 + 5) >> 1 = 4, T = 2: cubic; 32x32 is class 5, T = 0: Gaussian.  And the transposes.
@pytest.mark.parametrize("mode", (51, 49, 17, 19))
@pytest.mark.parametrize("gauss", (False, True), ids=("cubic", "gauss"))
def test_an_impulse_exposes_every_coefficient_with_its_sign(mode, gauss):
    """The main line is v everywhere but v + 64 at main[p]; side and corner are v.  With |A| = 1 the
    32 lines along the side direction run through every f, and sample (a, b) -- a along the main
    line -- reads ref[k-1 .. k+2], k = a + idx + 1; ref[p + 1] is main[p], so the tap t = p + 2 - k
    lands on the impulse and the sample is v + c[f][t], else v.  By hand, without the restatement's
    indexing."""
    vert = mode >= 34
    long_side, short = 32, (32 if gauss else 8)
    w, h = (short, long_side) if vert else (long_side, short)
    lw, lh = A._log2(w), A._log2(h)
    assert T.filter_gauss(lw, lh, mode) == gauss
    table = T.FG if gauss else T.FC
    ang = A.ANGLE[mode]
    assert abs(ang) == 1
    v, p = 300, 5
    top, left, corner = _lines(w, h, v)
    (top if vert else left)[0, p] += 64
    got = T.predict(top, left, corner, w, h, (mode,))[0, 0]
    seen_f, negative, positive = set(), 0, 0
    for b in range(long_side):
        d = (b + 1) * ang
        idx, f = d >> 5, d & 31
        seen_f.add(f)
        for a in range(short):
            t = p + 2 - (a + idx + 1)
            c = int(table[f][t]) if 0 <= t <= 3 else 0
            negative += c < 0
            positive += c > 0
            assert got[(b, a) if vert else (a, b)] == v + c, (mode, a, b, f, t)
    assert seen_f == set(range(32)) and positive > 60 and (negative > 30) == (not gauss)


def test_modes_18_and_50_equal_the_two_tap_outputs_everywhere():
    """f = 0 and G false in every size class: the identity, then the same PDPC."""
    rng = np.random.default_rng(18)
    for s in layout.SHAPES:
        n = 4
        top, left = rng.integers(0, 1024, (n, s.w + s.h)), rng.integers(0, 1024, (n, s.h + s.w))
        corner = rng.integers(0, 1024, n)
        got = T.predict(top, left, corner, s.w, s.h, (18, 50))
        want = A.predict(top[:, :s.w], left[:, :s.h], corner, s.w, s.h, (18, 50))
        assert np.array_equal(got, want), s.name


def test_modes_2_34_66_equal_the_two_tap_outputs_on_the_smallest_size_class_only():
    rng = np.random.default_rng(34)
    small, smoothed = 0, 0
    for s in layout.SHAPES:
        top, left = rng.integers(0, 1024, (3, s.w + s.h)), rng.integers(0, 1024, (3, s.h + s.w))
        corner = rng.integers(0, 1024, 3)
        got = T.predict(top, left, corner, s.w, s.h, (2, 34, 66))
        want = X.predict(top, left, corner, s.w, s.h, (2, 34, 66))
        if (A._log2(s.w) + A._log2(s.h)) >> 1 == 2:
            assert (s.w, s.h) in ((4, 4), (4, 8), (8, 4)) and np.array_equal(got, want), s.name
            small += 1
        else:
            assert all(not np.array_equal(got[q], want[q]) for q in range(3)), s.name
            smoothed += 1
    assert small >= 3 and smoothed >= 30
    # the smoothing by hand: mode 66 of an 8x8 CU, sample (i, j) is (ref[k-1] + 2 ref[k] + ref[k+1] + 2) >> 2, k = i + j + 2
    top, left, corner = rng.integers(0, 1024, (1, 16)), rng.integers(0, 1024, (1, 16)), np.array([7])
    got = T.predict(top, left, corner, 8, 8, (66,))[0, 0]
    ref = lambda k: int(top[0, min(k, 16) - 1])
    for j in range(8):
        for i in range(8):
            k = i + j + 2
            assert got[j, i] == (16 * ref(k - 1) + 32 * ref(k) + 16 * ref(k + 1) + 32) >> 6 == (ref(k - 1) + 2 * ref(k) + ref(k + 1) + 2) >> 2


def test_the_clip_below_0_and_above_1023():
    """Mode 60 (A = 16) of an 8x8 CU is cubic; its row 0 has f = 16, c = {-4, 36, 36, -4}, and sample
    i reads main[i-1 .. i+2].  On the line 1023 0 0 1023 1023 0 0 1023 ... sample 1 sums to -8184:
    P = -128, and sample 3 to 73656: P = 1151."""
    assert not T.filter_gauss(3, 3, 60) and A.ANGLE[60] == 16
    top = np.array([[1023, 0, 0, 1023] * 4], np.int64)
    left, corner = np.full((1, 16), 500, np.int64), np.array([500], np.int64)
    raw = T.predict(top, left, corner, 8, 8, (60,), clip=False)[0, 0]
    out = T.predict(top, left, corner, 8, 8, (60,))[0, 0]
    assert raw[0, 1] == (-4 * 1023 - 4 * 1023 + 32) >> 6 == -128 and raw[0, 3] == (2 * 36 * 1023 + 32) >> 6 == 1151
    assert out[0, 1] == 0 and out[0, 3] == 1023 and raw.min() < 0 and raw.max() > 1023
    assert np.array_equal(out, np.clip(raw, 0, 1023))


def test_angular_filter_for_every_shape_and_mode():
    """mip_angular_filter for the 47 shapes x 65 modes, thresholds spelled out by size class."""
    threshold = {2: 24, 3: 14, 4: 2, 5: 0, 6: 0}
    seen = set()
    for s in layout.SHAPES:
        lw, lh = A._log2(s.w), A._log2(s.h)
        for m in range(2, 67):
            want = int(min(abs(m - 50), abs(m - 18)) > threshold[(lw + lh) >> 1])
            assert mipgpu.angular_filter(lw, lh, m) == want == int(T.filter_gauss(lw, lh, m)), (s.name, m)
        seen.add((lw + lh) >> 1)
    assert seen == {2, 3, 4, 5, 6} and len(layout.SHAPES) == 47
    assert [mipgpu.angular_filter(3, 3, m) for m in (2, 3, 4, 18, 32, 33, 34, 35, 36, 50, 64, 65, 66)] == [1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 1]
    assert mipgpu.angular_filter(2, 2, 2) == 0 and mipgpu.angular_filter(6, 6, 19) == 1 and mipgpu.angular_filter(4, 4, 20) == 0
    lib = mipgpu.library()
    for bad in ((1, 3, 18), (3, 7, 18), (3, 3, 1), (3, 3, 67)):
        assert lib.mip_angular_filter(*bad) < 0 and b"angular filter" in lib.mip_last_error(), bad
        with pytest.raises(mipgpu.MipError):
            mipgpu.angular_filter(*bad)


# ---------------------------------------------------------------- the host walks
@pytest.fixture(scope="module")
def tap4_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("angular_tap4") / "test_angular_tap4"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "vvc-mip-gpu_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", str(exe),
                           os.path.join(REPO, "tests", "cpp", "test_angular_tap4.cpp")])
    return str(exe)


JOBS = ((None, 0), (TC.ODD_LENGTH_LIST, 0), (TC.EVEN_MODES, 1), (RR.SPARSE_MODES, 3))
SWEEP_JOBS = ((TC.SWEEP_LIST, 0), (RR.SPARSE_MODES, 2))      # (short lists: the program runs under two sanitizers)


def _decisions(ang_cost, un, seed):
    rng = np.random.default_rng(seed)
    near = np.where(ang_cost == UN, 0, ang_cost)
    best_cost = (near + rng.integers(-40, 41, near.shape) * rng.integers(0, 2, near.shape)).clip(0).astype(np.int32)
    best_mode = rng.choice(np.array([0, 3, 11, 0xF0, 0xF1], np.uint8), best_cost.shape)
    dead = np.broadcast_to(un, best_cost.shape) | (rng.random(best_cost.shape) < 0.05)
    best_cost[dead], best_mode[dead] = UN, 0xFF
    return best_mode, best_cost


def _run_walks(exe, tmp_path, jobs, frames, refs, un, extended, e_top, e_left, best_mode, best_cost, bias):
    nf, h, w = frames.shape
    ncu = un.size
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([w, h, nf, bias, len(jobs), int(extended)], np.int32).tobytes())
        for a, dt in ((frames, np.uint16), (refs, np.uint16), (un, np.uint8), (e_top, np.uint8), (e_left, np.uint8),
                      (best_mode, np.uint8), (best_cost, np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
        for modes, seeds in jobs:
            modes = () if modes is None else modes
            f.write(np.array([seeds, len(modes)], np.int32).tobytes() + np.array(modes, np.uint8).tobytes())
    r = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "angular_tap4: ok" in r.stdout, (r.returncode, r.stdout + r.stderr)
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


def _walks_equal_the_restatement(exe, tmp_path, jobs, frames, refs, un, refs_setting, full):
    """frames / refs [n, H, W]; full: the restatement's 65-mode tables [n, ncu, 65] with the pair."""
    _, h, w = frames.shape
    got_top, got_left = mipgpu.extended_refs(w, h)             # (the program ignores them under SUB)
    best_mode, best_cost = _decisions(full["ang_cost"], un, w)
    outs = _run_walks(exe, tmp_path, jobs, frames, refs, un, refs_setting == TC.EXT, got_top, got_left, best_mode, best_cost, 7)
    for (modes, seeds), out in zip(jobs, outs):
        if seeds:
            want = RR.refine(full, modes, seeds)
            assert np.array_equal(out["tried"], want["tried"]), (modes, seeds)
        else:
            want = full if modes is None else TC.listed(full, modes)
            assert np.all(out["tried"] == 0x5A)
        for key in TC.TABLES + ("ang_mode", "ang_cost"):
            assert np.array_equal(out[key], want[key]), (modes, seeds, key)
        mode, cost = A.merge(best_mode, best_cost, want["ang_mode"], want["ang_cost"], 7)
        assert np.array_equal(out["best_mode"], mode) and np.array_equal(out["best_cost"], cost), (modes, seeds)


@needs_gxx
@pytest.mark.parametrize("refs_setting", (TC.EXT, TC.SUB), ids=("extended", "substituted"))
def test_host_walks_equal_the_restatement(tap4_exe, tmp_path, refs_setting):
    """264x136, one frame: angular_frames_host and angular_refine_frames_host with
    MIP_ANG_INTERP_4TAP (all 65 modes, the odd-length list, refined searches) against the
    restatement; inside the program ang_sample_tap4 is held to the block step's SAD."""
    f, refs, un, _, _, full = TC.case(W, H, refs_setting, None, 1)
    _walks_equal_the_restatement(tap4_exe, tmp_path, JOBS, f, refs, un, refs_setting, full)


@needs_gxx
@pytest.mark.parametrize("size", size_sweep.ALL_SIZES[::5], ids=size_sweep.size_id)
def test_host_walks_at_every_fifth_sweep_size(tap4_exe, tmp_path, size):
    """One noise frame per size, both reference settings: a plain walk and a refined search."""
    w, h = size
    for refs_setting in (TC.EXT, TC.SUB):
        frame, un, _, _, tabs = TC.sweep_case(w, h, refs_setting)
        full = {k: v[None] for k, v in tabs.items()}
        _walks_equal_the_restatement(tap4_exe, tmp_path, SWEEP_JOBS, frame[None], frame[None], un, refs_setting, full)


@needs_gxx
def test_tables_and_filter_choice_of_the_plan_header(tap4_exe):
    """ang_filter_gauss and the coefficient words as ang_coef unpacks them, printed by the program."""
    r = subprocess.run([tap4_exe, "tables"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    at = 0
    for lw in range(2, 7):
        for lh in range(2, 7):
            assert lines[at] == "".join("01"[T.filter_gauss(lw, lh, m)] for m in range(2, 67)), (lw, lh)
            at += 1
    got = np.array([[int(v) for v in ln.split()] for ln in lines[at:at + 64]])
    assert np.array_equal(got[:32], T.FC) and np.array_equal(got[32:], T.FG)


# ---------------------------------------------------------------- interface
def _header():
    with open(os.path.join(REPO, "include", "mipgpu.h")) as f:
        return f.read()


def test_header_and_python_constants():
    src = _header()
    assert re.search(r"#define MIP_ANG_INTERP_2TAP 0\b", src) and mipgpu.ANG_INTERP_2TAP == T.INTERP_2TAP == 0
    assert re.search(r"#define MIP_ANG_INTERP_4TAP 1\b", src) and mipgpu.ANG_INTERP_4TAP == T.INTERP_4TAP == 1
    for name in ("ANG_INTERP_2TAP", "ANG_INTERP_4TAP", "angular_filter"):
        assert name in mipgpu.__all__, name
    assert isinstance(mipgpu.MipEngine.angular_interp, property) and mipgpu.MipEngine.angular_interp.fset is not None
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int mip_angular_interp\(mip_engine \*e, int interp\);", code)
    assert re.search(r"int mip_angular_interp_get\(const mip_engine \*e\);", code)
    assert re.search(r"int mip_angular_filter\(int lw, int lh, int mode\);", code)
    assert re.search(r"#define MIPGPU_ABI_VERSION 7\b", src) and mipgpu.library().mip_abi_version() == 7
    # the contract's tables stand in the header as the restatement has them
    text = re.sub(r"\s*\*\s*", " ", src)
    assert "T[0..6] = {24, 24, 24, 14, 2, 0, 0}" in text and "fG[f] = {16 - (f>>1), 32 - (f>>1), 16 + (f>>1), f>>1}" in text
    rows = re.findall(r"\{ ?(-?\d+), ?(-?\d+), ?(-?\d+), ?(-?\d+)\}", text[text.index("fC[f] for f = 0..16"):text.index("fC[32 - f] is fC[f] reversed")])
    assert np.array_equal(np.array(rows, int), T.FC[:17])
    # the paragraph of what is not modelled no longer lists the filters or the smoothing as missing
    para = text[text.index("NOT modelled: wide-angle"):text.index("Exactly mip_intra_device's: SAD")]
    assert "4-tap" not in para and "reference smoothing" not in para and "leaves the last sample of its 2M-long line unsmoothed" in para


def test_switch_refuses_bad_arguments():
    lib = mipgpu.library()
    assert lib.mip_angular_interp(None, 1) != 0 and b"engine is NULL" in lib.mip_last_error()
    assert lib.mip_angular_interp_get(None) < 0 and b"engine is NULL" in lib.mip_last_error()
    # without a GPU no engine exists; the value rule is in the text of mip_angular_interp (the GPU test exercises it on an engine)
    with open(os.path.join(REPO, "vvc-mip-gpu_amd", "csrc", "mipgpu.cpp")) as f:
        src = f.read()
    body = src[src.index("int mip_angular_interp(mip_engine *e, int interp) {"):src.index("int mip_angular_interp_get(")]
    assert "interp != MIP_ANG_INTERP_2TAP && interp != MIP_ANG_INTERP_4TAP" in body and "unknown angular interpolation setting" in body
    assert "std::lock_guard<std::recursive_mutex> lk(e->mu);" in body and body.index("lock_guard") < body.index("ang_interp.store")


def test_pinned_signatures_are_untouched():
    assert list(inspect.signature(mipgpu.MipEngine.angular_refine).parameters) == ["self", "frames", "refs", "modes", "seeds", "table"]
    assert list(inspect.signature(mipgpu.MipEngine.angular_refine_device).parameters) == [
        "self", "frames", "modes", "seeds", "cost", "sad", "satd", "ang_mode", "ang_cost", "tried", "refs", "bias", "best_mode", "best_cost",
        "stream"]
    assert list(inspect.signature(mipgpu.MipEngine.angular_device).parameters) == [
        "self", "frames", "modes", "cost", "sad", "satd", "ang_mode", "ang_cost", "refs", "bias", "best_mode", "best_cost", "stream"]
    assert list(inspect.signature(mipgpu.MipEngine.predicted_frames_ex).parameters) == [
        "self", "frames", "penalty", "bias", "refs", "angular", "angular_bias"]
    assert list(inspect.signature(mipgpu.MipEngine.angular).parameters) == ["self", "frames", "refs", "modes", "table"]
    assert list(inspect.signature(mipgpu.extended_refs).parameters) == ["width", "height", "filter"]
    assert isinstance(mipgpu.MipEngine.angular_refs, property)
    lib = mipgpu.library()
    assert len(lib.mip_angular_device.argtypes) == 15 and len(lib.mip_angular_refine_device.argtypes) == 17
    assert len(lib.mip_predict_device_ex.argtypes) == 11 and len(lib.mip_candidates_frames.argtypes) == 13
    assert len(lib.mip_predicted_frames_ex.argtypes) == 16 and len(lib.mip_angular_frames.argtypes) == 9
    assert lib.mip_angular_refs.argtypes == [ctypes.c_void_p, ctypes.c_int] == lib.mip_angular_interp.argtypes
    assert lib.mip_angular_filter.argtypes == [ctypes.c_int] * 3


def test_dispatch_reads_both_settings_once_per_launch():
    """predict_launch and angular_device_impl each read the interpolation setting once, next to
    their one read of the reference setting; the chains (mip_predicted_frames_ex,
    mip_candidates_frames) have no read of their own: they go through those two functions."""
    with open(os.path.join(REPO, "vvc-mip-gpu_amd", "csrc", "host_stages.cpp")) as f:
        host = f.read()
    launch = host[host.index("static int predict_launch("):host.index("static int predict_args_ok(")]
    impl = host[host.index("static int angular_device_impl("):host.index("int mip_angular_device(")]
    for part, calls in ((launch, ("launch_predict_angular_tap4(x, s)",)), (impl, ("launch_angular_tap4_refine(a, s)", "launch_angular_tap4(a, s)"))):
        assert part.count("e->ang_interp.load()") == 1 and part.count("e->ang_refs.load()") == 1
        assert abs(part.index("e->ang_interp.load()") - part.index("e->ang_refs.load()")) < 200
        for call in calls:
            assert call in part, call
    assert host.count("ang_interp") == 2
    for name in ("host_pipeline.cpp", "mipgpu.cpp"):
        with open(os.path.join(REPO, "vvc-mip-gpu_amd", "csrc", name)) as f:
            assert "ang_interp.load()" not in f.read().replace("return e->ang_interp.load();", ""), name


# ---------------------------------------------------------------- kernel resources
def _kernel(name):
    found = [v for k, v in kernel_resources.kernels(mipgpu.LIB_PATH).items() if re.search(r"\d+%sE" % name, k)]
    assert len(found) == 1, name
    return found[0]


def test_kernel_resources():
    """The three 4-tap kernels: no scratch, no spilled vector register; the two cost kernels three
    waves per SIMD like their siblings (at most 168 VGPRs, 3 x LDS <= 160 KB); the 64 coefficient
    words add 256 bytes of LDS to the _ext kernels' (DESIGN.md section 5.12), and no other kernel of
    the family pays for them.  The VGPR figures themselves are pinned in
    tests/test_kernel_resources.py."""
    mipgpu.library()
    want = {"angular_tap4_kernel": 13968, "angular_tap4_refine_kernel": 14268, "angular_tap4_predict_kernel": 5632}
    for name, lds in want.items():
        k = _kernel(name)
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, name
        assert k[".group_segment_fixed_size"] == lds, name
    for name in ("angular_tap4_kernel", "angular_tap4_refine_kernel"):
        k = _kernel(name)
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 168 and 3 * k[".group_segment_fixed_size"] <= 160 * 1024
    others = {"angular_kernel": 13308, "angular_refine_kernel": 13612, "angular_ext_kernel": 13708,
              "angular_ext_refine_kernel": 14012, "angular_ext_predict_kernel": 5376, "angular_predict_kernel": 4352}
    for name, lds in others.items():
        k = _kernel(name)
        assert (k[".group_segment_fixed_size"], k[".private_segment_fixed_size"]) == (lds, 0), name
    # the 4-tap kernels' names stay clear of the patterns other tests find their siblings by
    new = [name for name in kernel_resources.kernels(mipgpu.LIB_PATH) if "_tap4_" in name]
    assert len(new) == 3
    for name in new:
        assert not re.search(r"\d+(angular_kernel|angular_refine_kernel|angular_ext_kernel|angular_ext_refine_kernel|"
                             r"angular_ext_predict_kernel|angular_predict_kernel|intra_kernel)E", name), name
        assert not any(part in name for part in ("filter_kernel", "mip_search_kernel", "candidates_kernel")), name


# ---------------------------------------------------------------- non-vacuity of the GPU cases
def _taps(w, h, m):
    want = {}
    T.predict(*_lines(w, h, 1), w, h, (m,), want=want)
    return want[m]


def test_gpu_case_set_is_not_vacuous():
    """On the restatements alone, for the frames and lists of tests/test_gpu_angular_tap4.py.

    Both filters occur for every fractional mode among the shapes of the compared (available) CUs.
    The k - 1 = 0 corner tap is read for A >= 0.  A tap lands on the clamp at M (a CU without an
    extension) and at M' > M (a CU with a partial one).  A negative-angle tap lands on the side's cap,
    which no tap of the 2-tap predictor does in mode 34.  Of the fractional-mode table entries of
    available CUs, 90.2 % (extended lines) and 88.8 % (substituted lines) differ from the 2-tap tables
    (measured on these frames); at least half of that is asserted."""
    _, _, un, e_top, e_left, tap4 = TC.case(W, H, TC.EXT)
    x, y, bw, bh = _geometry(W, H)
    on = ~un
    shapes = {(int(a), int(b)) for a, b in zip(bw[on], bh[on])}
    assert len(shapes) == 17 and {(A._log2(w) + A._log2(h)) >> 1 for w, h in shapes} == {2, 3, 4, 5, 6}
    for m in T.FRACTIONAL_MODES:
        kinds = {bool(T.filter_gauss(A._log2(w), A._log2(h), m)) for w, h in shapes}
        assert kinds == {False, True}, m
    assert set(TC.ODD_LENGTH_LIST) & set(T.FRACTIONAL_MODES) and {2, 18, 34, 50, 66} <= set(TC.ODD_LENGTH_LIST) and len(TC.ODD_LENGTH_LIST) % 2
    # the corner tap for A >= 0: tap 0 of sample (0, 0) has k - 1 = 0 in every mode with 0 <= A < 32
    for m in (3, 17, 18, 50, 51, 65):
        t = _taps(8, 8, m)
        assert A.ANGLE[m] >= 0 and t["k"][0, 0, 0] == 0 and t["pos"][0, 0, 0] == t["S"], m
    assert _taps(8, 8, 66)["k"].min() == 1 and _taps(8, 8, 2)["k"].min() == 1     # (A = 32: never)
    # the clamp at M and at M' > M: mode 66 (vertical class), k + 2 reaches w + h + 2
    k66 = lambda w, h: _taps(w, h, 66)["k"].max()
    plain = on & (e_top == 0) & (x + bw <= W)
    partial = on & (e_top > 0) & (e_top < bh)
    full = on & (e_top == bh)
    assert plain.any() and partial.any() and full.any()
    for sel in (plain, partial, full):
        c = int(np.nonzero(sel)[0][0])
        assert k66(int(bw[c]), int(bh[c])) == bw[c] + bh[c] + 2 > bw[c] + e_top[c]
    part_left = on & (e_left > 0) & (e_left < bw)
    c = int(np.nonzero(part_left)[0][0])
    assert _taps(int(bw[c]), int(bh[c]), 2)["k"].max() == bw[c] + bh[c] + 2 > bh[c] + e_left[c]
    # the side's cap: mode 34 (A = -32, inv = 512), tap k - 1 = -h at sample (0, h - 1) projects to p = h = S
    for w, h in ((4, 4), (8, 16), (32, 8)):
        t = _taps(w, h, 34)
        p = (-t["k"] * t["inv"] + 256) >> 9
        assert t["S"] == h and p[0].max() == h and p[1].max() == h - 1 and t["pos"].min() == 0
    t = _taps(16, 8, 19)                                                            # a fractional one reaches it too
    assert ((-t["k"][0] * t["inv"] + 256) >> 9).max() >= t["S"]
    # how much differs from the 2-tap tables
    slots = np.array(T.FRACTIONAL_MODES) - 2
    two = XC.case(W, H)[5]
    share = (tap4["cost"][:, on][:, :, slots] != two["cost"][:, on][:, :, slots]).mean()
    assert share >= 0.902 / 2, share
    sub4, sub2 = TC.case(W, H, TC.SUB)[5], XC.substituted(W, H)
    share = (sub4["cost"][:, on][:, :, slots] != sub2["cost"][:, on][:, :, slots]).mean()
    assert share >= 0.888 / 2, share
    # the two reference settings differ under the 4-tap filter as well -- in the negative-angle modes
    # too, whose tap k + 2 reaches ref[M + 1]; modes 18 and 50 (the identity) stay
    assert not np.array_equal(tap4["cost"][:, :, :16], sub4["cost"][:, :, :16]) and not np.array_equal(tap4["cost"][:, :, 17:48], sub4["cost"][:, :, 17:48])
    assert np.array_equal(tap4["cost"][:, :, 16], sub4["cost"][:, :, 16]) and np.array_equal(tap4["cost"][:, :, 48], sub4["cost"][:, :, 48])
    plain = (e_top == 0) & (e_left == 0)
    assert np.array_equal(tap4["cost"][:, plain], sub4["cost"][:, plain])
