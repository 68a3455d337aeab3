"""Extended angular reference lines on the CPU (no GPU): the numpy restatement
tests/angular_ext_ref.py pinned by hand-checkable cases (an anti-diagonal frame f(x + y) that modes
66 and 2 predict exactly where the line is fully extended, and nowhere with substituted lines);
mip_extended_refs against the restatement's lengths at every size of tests/size_sweep.py for the
MIP_FILTER_NONE set and the eight filters, with the prefix and window facts the kernels' staging
relies on; the C++ host walks of csrc/angular_plan.h, compiled stand-alone with
-fsanitize=address,undefined (tests/cpp/test_angular_ext.cpp), against the restatement bit for bit;
the header's and the binding's constants, the switch's argument rules and the pinned signatures;
the new kernels' resources in the built library; and the coverage conditions of the GPU cases."""
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
import kernel_resources
import mipgpu
import size_sweep
from mipgpu import layout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UN = layout.UNAVAILABLE
W, H = XC.SIZE
ALL_SETS = (None,) + tuple(mipgpu.FILTERS)

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _geometry(w, h):
    _, x, y, bw, bh = layout.cu_geometry(w, h, np.arange(layout.num_ctus(w, h) * layout.CUS_PER_CTU))
    return x, y, bw, bh


# ---------------------------------------------------------------- hand-checkable cases
def _antidiagonal(w, h, seed=0x66):
    f = np.random.default_rng(seed).integers(0, 1024, w + h + 1)
    return f[np.arange(w)[None, :] + np.arange(h)[:, None]].astype(np.uint16)


def test_order_key_is_z_scan_inside_ctu_raster():
    """By hand: inside a CTU the 4x4 blocks (0,0) (1,0) (0,1) (1,1) (2,0) have Morton codes 0 1 2 3 4;
    the block right of an 8x8 quad's top-right block comes later, the one below-left of its
    bottom-left earlier only across a 16x16 boundary; any sample of an earlier CTU comes first."""
    key = lambda sx, sy: int(X.order_key(sx, sy, 264))
    assert [key(sx, sy) for sx, sy in ((0, 0), (4, 0), (0, 4), (4, 4), (8, 0))] == [0, 1, 2, 3, 4]
    assert key(3, 3) == key(0, 0) and key(127, 127) == 1023 and key(128, 0) == 1024 and key(0, 128) == 3 * 1024
    assert key(8, 3) > key(4, 4)                      # above-right of the block at (4, 4) ... is coded later
    assert key(8, 3) < key(8, 4)                      # ... but precedes the block below it
    assert key(7, 8) > key(8, 4)                      # z-scan: the 8x8 quad at (0, 8) follows the quad at (8, 0)
    assert key(127, 131) > key(128, 124)              # the CTU below follows every CTU of the row above
    assert key(255, 127) < key(0, 128)


def test_antidiagonal_frame_is_predicted_exactly_where_the_line_is_real():
    """f(x + y) at 264x136: mode 66 predicts top[i + j + 1] and mode 2 left[i + j + 1], which IS the
    frame wherever those samples are real: SAD 0 for the 4387 available CUs with E_top = h and the
    2199 with E_left = w.  With substituted lines none of them reaches 0."""
    frame = _antidiagonal(W, H)
    un, e_top, e_left = XC.lengths(W, H)
    x, y, bw, bh = _geometry(W, H)
    assert (~un).sum() == 16658 and (~un & (x + bw > W)).sum() == 5229
    ext = X.tables(frame, frame, un, e_top, e_left, (2, 66))
    sub = A.tables(frame, frame, un, (2, 66))
    full_top, full_left = ~un & (e_top == bh), ~un & (e_left == bw)
    assert full_top.sum() == 4387 and full_left.sum() == 2199
    assert not ext["sad"][full_top, 64].any() and not ext["sad"][full_left, 0].any()
    assert np.all(sub["sad"][full_top, 64] > 0) and np.all(sub["sad"][full_left, 0] > 0)
    # a CU with E_top = h predicts mode 66 as top[i + j + 1] exactly: one CU by hand
    k = int(np.nonzero(full_top & (bw == 8) & (bh == 8))[0][5])
    want = frame[y[k] - 1, x[k] + 1 + np.arange(8)[None, :] + np.arange(8)[:, None]]
    assert np.array_equal(X.predict_cu(frame, x[k], y[k], 8, 8, e_top[k], e_left[k], 66), want)


def test_modes_18_to_50_and_unextended_cus_equal_the_substituted_restatement():
    _, _, un, e_top, e_left, ext = XC.case(W, H)
    sub = XC.substituted(W, H)
    plain = (e_top == 0) & (e_left == 0)
    assert (plain & ~un).sum() > 1000
    for key in XC.TABLES:
        assert np.array_equal(ext[key][:, :, 16:49], sub[key][:, :, 16:49]), key          # modes 18..50
        assert np.array_equal(ext[key][:, plain], sub[key][:, plain]), key
    # a top extension changes no horizontal mode, a left extension no vertical mode
    assert np.array_equal(ext["sad"][:, e_left == 0, :16], sub["sad"][:, e_left == 0, :16])
    assert np.array_equal(ext["sad"][:, e_top == 0, 49:], sub["sad"][:, e_top == 0, 49:])


# ---------------------------------------------------------------- the length rule
@pytest.fixture(scope="module")
def ext_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("angular_ext") / "test_angular_ext"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "vvc-mip-gpu_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", str(exe),
                           os.path.join(REPO, "tests", "cpp", "test_angular_ext.cpp")])
    return str(exe)


def _window_facts(w, h, e_top, e_left):
    """What the kernels' staging relies on: where an extension can end, for a CU inside a 32x32
    block at (x0, y0) and for the 64x64 CU (the same with 64 / 128)."""
    x, y, bw, bh = _geometry(w, h)
    side = np.where((bw == 64) & (bh == 64), 64, 32)
    x0, y0 = x - x % side, y - y % side
    top_end, left_end = x + bw + e_top, y + bh + e_left
    t, l = e_top > 0, e_left > 0
    assert np.all(top_end[t & (y != y0)] <= (x0 + side)[t & (y != y0)])
    assert np.all(top_end[t & (y == y0)] <= (x0 + 2 * side)[t & (y == y0)])
    below = l & (left_end > y0 + side)
    assert np.all(x[below] == x0[below]) and np.all(left_end[l] <= (y0 + 2 * side)[l])
    assert np.all(e_top <= bh) and np.all(e_left <= bw)


@pytest.mark.parametrize("size", size_sweep.ALL_SIZES + [XC.SIZE], ids=size_sweep.size_id)
def test_extended_refs_equal_the_restatement_at_every_sweep_size(size):
    """mip_extended_refs for the MIP_FILTER_NONE set and the eight filters; the restatement runs
    once per distinct (availability set, undefined set) of the size.  The usable samples of a line
    form a prefix, without a filter both lengths are multiples of 4, and the window facts hold."""
    w, h = size
    seen = {}
    for filt in ALL_SETS:
        un = mipgpu.unavailable_cus(w, h, filt)
        und = XC.undefined(w, h, filt)
        key = (un.tobytes(), None if und is None or not und.any() else und.tobytes())
        if key not in seen:
            top, left = X.usable(w, h, un, und)
            e_top, e_left = np.cumprod(top, axis=1).sum(axis=1), np.cumprod(left, axis=1).sum(axis=1)
            assert np.array_equal(top.sum(axis=1), e_top) and np.array_equal(left.sum(axis=1), e_left)       # a prefix
            _window_facts(w, h, e_top, e_left)
            if key[1] is None:
                assert not (e_top % 4).any() and not (e_left % 4).any()
            assert not e_top[un].any() and not e_left[un].any()
            seen[key] = (e_top, e_left)
        got_top, got_left = mipgpu.extended_refs(w, h, filt)
        assert got_top.dtype == np.uint8 and np.array_equal(got_top, seen[key][0]) and np.array_equal(got_left, seen[key][1]), filt


@pytest.mark.parametrize("size", ((1920, 1080), (416, 240), (256, 256), (132, 132)), ids=size_sweep.size_id)
def test_window_facts_at_the_larger_sizes(size):
    w, h = size
    top, left = mipgpu.extended_refs(w, h)
    _window_facts(w, h, top.astype(np.int64), left.astype(np.int64))
    assert not (top % 4).any() and not (left % 4).any()


def test_lengths_at_the_gpu_size():
    """264x136: of the CUs inside the frame 51 % have a top and 31 to 32 % a left extension, and about 1400
    on each line a partial one."""
    un, e_top, e_left = XC.lengths(W, H)
    x, y, bw, bh = _geometry(W, H)
    inside = ~un & (x + bw <= W)
    assert inside.sum() == 16658 - 5229
    assert 0.50 < (e_top[inside] > 0).mean() < 0.52 and 0.31 < (e_left[inside] > 0).mean() < 0.33
    assert 1200 < ((e_top > 0) & (e_top < bh)).sum() < 1600 and 1200 < ((e_left > 0) & (e_left < bw)).sum() < 1600
    assert not e_top[~inside].any() and not e_left[~inside].any()


@needs_gxx
@pytest.mark.parametrize("size", size_sweep.ALL_SIZES[::5] + [XC.SIZE], ids=size_sweep.size_id)
def test_no_extension_holds_an_undefined_filtered_sample(ext_exe, tmp_path, size):
    """From work_plan.h's own undefined set (filter_poison), in the stand-alone program: every sample
    of every extension mip_extended_refs reports lies inside the frame and outside that set, for the
    NONE set and the eight filters; the lengths are ang_ext_lengths over it."""
    w, h = size
    looked = 0
    for index, filt in enumerate(ALL_SETS):
        top, left = mipgpu.extended_refs(w, h, filt)
        src = tmp_path / "lengths.bin"
        with open(src, "wb") as f:
            f.write(np.array([w, h, index - 1], np.int32).tobytes() + top.tobytes() + left.tobytes())
        r = subprocess.run([ext_exe, "undefined", str(src)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "undefined: ok" in r.stdout, (filt, r.returncode, r.stdout + r.stderr)
        looked += int(r.stdout.split()[-1])
    assert looked == 0 or looked > 1000
    assert looked or min(w, h) < 12


# ---------------------------------------------------------------- the host walks
JOBS = ((None, 0), (XC.ODD_LENGTH_LIST, 0), (XC.EVEN_MODES, 1), (XC.EVEN_MODES, 3), (RR.SPARSE_MODES, 2))


def _decisions(ang_cost, un, seed):
    rng = np.random.default_rng(seed)
    near = np.where(ang_cost == UN, 0, ang_cost)
    best_cost = (near + rng.integers(-40, 41, near.shape) * rng.integers(0, 2, near.shape)).clip(0).astype(np.int32)
    best_mode = rng.choice(np.array([0, 3, 11, 0xF0, 0xF1], np.uint8), best_cost.shape)
    dead = np.broadcast_to(un, best_cost.shape) | (rng.random(best_cost.shape) < 0.05)
    best_cost[dead], best_mode[dead] = UN, 0xFF
    return best_mode, best_cost


def _run_walks(exe, tmp_path, frames, refs, un, e_top, e_left, best_mode, best_cost, bias):
    nf, h, w = frames.shape
    ncu = un.size
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([w, h, nf, bias, len(JOBS)], np.int32).tobytes())
        for a, dt in ((frames, np.uint16), (refs, np.uint16), (un, np.uint8), (e_top, np.uint8), (e_left, np.uint8),
                      (best_mode, np.uint8), (best_cost, np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
        for modes, seeds in JOBS:
            modes = () if modes is None else modes
            f.write(np.array([seeds, len(modes)], np.int32).tobytes() + np.array(modes, np.uint8).tobytes())
    r = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "angular_ext: ok" in r.stdout, (r.returncode, r.stdout + r.stderr)
    raw = open(dst, "rb").read()
    table = (np.int32, nf * ncu * 65, (nf, ncu, 65))
    per_cu = lambda dt: (dt, nf * ncu, (nf, ncu))
    outs, at = [], 0
    for _ in JOBS:
        out = {}
        for key, (dt, count, shape) in (("cost", table), ("sad", table), ("satd", table), ("ang_mode", per_cu(np.uint8)),
                                        ("ang_cost", per_cu(np.int32)), ("tried", per_cu(np.uint8)), ("best_mode", per_cu(np.uint8)),
                                        ("best_cost", per_cu(np.int32))):
            out[key] = np.frombuffer(raw, dt, count, at).reshape(shape)
            at += count * np.dtype(dt).itemsize
        outs.append(out)
    assert at == len(raw)
    return outs


@needs_gxx
@pytest.mark.parametrize("size, frames", ((XC.SIZE, 1), ((132, 132), 2)), ids=("264x136", "132x132"))
def test_host_walks_equal_the_restatement(ext_exe, tmp_path, size, frames):
    """angular_frames_host and angular_refine_frames_host with the lengths of mip_extended_refs: all
    65 modes, an odd-length list, and refined searches, against the restatement (the refinement rule
    of tests/angular_refine_ref.py over the extended 65-mode tables); the per-sample predictor is
    held to the walks' SAD inside the program."""
    w, h = size
    f, refs, un, e_top, e_left, full = XC.case(w, h, None, frames)
    got_top, got_left = mipgpu.extended_refs(w, h)
    best_mode, best_cost = _decisions(full["ang_cost"], un, w)
    outs = _run_walks(ext_exe, tmp_path, f, refs, un, got_top, got_left, best_mode, best_cost, 7)
    for (modes, seeds), out in zip(JOBS, outs):
        if seeds:
            want = RR.refine(full, modes, seeds)
            assert np.array_equal(out["tried"], want["tried"]), (modes, seeds)
        else:
            want = full if modes is None else XC.listed(full, modes)
            assert np.all(out["tried"] == 0x5A)
        for key in XC.TABLES + ("ang_mode", "ang_cost"):
            assert np.array_equal(out[key], want[key]), (modes, seeds, key)
        mode, cost = A.merge(best_mode, best_cost, want["ang_mode"], want["ang_cost"], 7)
        assert np.array_equal(out["best_mode"], mode) and np.array_equal(out["best_cost"], cost), (modes, seeds)


# ---------------------------------------------------------------- interface
def _header():
    with open(os.path.join(REPO, "include", "mipgpu.h")) as f:
        return f.read()


def test_header_and_python_constants():
    src = _header()
    assert re.search(r"#define MIP_ANG_REFS_SUBSTITUTED 0\b", src) and mipgpu.ANG_REFS_SUBSTITUTED == X.SUBSTITUTED == 0
    assert re.search(r"#define MIP_ANG_REFS_EXTENDED +1\b", src) and mipgpu.ANG_REFS_EXTENDED == X.EXTENDED == 1
    for name in ("ANG_REFS_SUBSTITUTED", "ANG_REFS_EXTENDED", "extended_refs"):
        assert name in mipgpu.__all__, name
    assert isinstance(mipgpu.MipEngine.angular_refs, property) and mipgpu.MipEngine.angular_refs.fset is not None
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int mip_angular_refs\(mip_engine \*e, int refs\);", code)
    assert re.search(r"int mip_angular_refs_get\(const mip_engine \*e\);", code)
    assert re.search(r"int mip_extended_refs\(int width, int height, int filter, uint8_t \*top_out, uint8_t \*left_out\);", code)
    assert re.search(r"#define MIPGPU_ABI_VERSION 7\b", src) and mipgpu.library().mip_abi_version() == 7
    text = re.sub(r"\s*\*\s*", " ", src)
    assert "availability below binary / ternary splits is z-order" in text and "THE MODEL" in text


def test_switch_and_lengths_refuse_bad_arguments():
    lib = mipgpu.library()
    assert lib.mip_angular_refs(None, 1) != 0 and b"engine is NULL" in lib.mip_last_error()
    assert lib.mip_angular_refs_get(None) < 0 and b"engine is NULL" in lib.mip_last_error()
    out = np.zeros(layout.num_ctus(136, 72) * layout.CUS_PER_CTU, np.uint8)
    assert lib.mip_extended_refs(136, 72, -1, None, None) != 0
    assert lib.mip_extended_refs(136, 72, 8, out.ctypes.data, None) != 0 and b"invalid filter" in lib.mip_last_error()
    assert lib.mip_extended_refs(134, 72, -1, out.ctypes.data, None) != 0
    assert lib.mip_extended_refs(136, 72, -1, out.ctypes.data, None) == 0 and out.any()          # either output alone
    left = np.zeros_like(out)
    assert lib.mip_extended_refs(136, 72, -1, None, left.ctypes.data) == 0 and left.any()
    top, both = mipgpu.extended_refs(136, 72)
    assert np.array_equal(top, out) and np.array_equal(both, left)


def test_a_bad_setting_is_refused_by_the_rule_the_library_uses():
    """Without a GPU no engine exists; the value rule is in the text of mip_angular_refs (the GPU
    test exercises it on an engine)."""
    with open(os.path.join(REPO, "vvc-mip-gpu_amd", "csrc", "mipgpu.cpp")) as f:
        src = f.read()
    body = src[src.index("int mip_angular_refs(mip_engine *e, int refs) {"):src.index("int mip_angular_refs_get(")]
    assert "refs != MIP_ANG_REFS_SUBSTITUTED && refs != MIP_ANG_REFS_EXTENDED" in body and "unknown angular reference setting" in body


def test_pinned_signatures_are_untouched():
    assert list(inspect.signature(mipgpu.MipEngine.angular_refine).parameters) == ["self", "frames", "refs", "modes", "seeds", "table"]
    assert list(inspect.signature(mipgpu.MipEngine.angular_refine_device).parameters) == [
        "self", "frames", "modes", "seeds", "cost", "sad", "satd", "ang_mode", "ang_cost", "tried", "refs", "bias", "best_mode", "best_cost",
        "stream"]
    assert list(inspect.signature(mipgpu.MipEngine.predicted_frames_ex).parameters) == [
        "self", "frames", "penalty", "bias", "refs", "angular", "angular_bias"]
    assert list(inspect.signature(mipgpu.MipEngine.angular).parameters) == ["self", "frames", "refs", "modes", "table"]
    lib = mipgpu.library()
    assert len(lib.mip_angular_device.argtypes) == 15 and len(lib.mip_angular_refine_device.argtypes) == 17
    assert len(lib.mip_predict_device_ex.argtypes) == 11 and len(lib.mip_candidates_frames.argtypes) == 13
    assert lib.mip_angular_refs.argtypes == [ctypes.c_void_p, ctypes.c_int]


# ---------------------------------------------------------------- kernel resources
def _kernel(name):
    found = [v for k, v in kernel_resources.kernels(mipgpu.LIB_PATH).items() if re.search(r"\d+%sE" % name, k)]
    assert len(found) == 1, name
    return found[0]


def test_kernel_resources():
    """The three _ext kernels: no scratch, no spilled vector register; the two cost kernels three
    waves per SIMD like their siblings (at most 168 VGPRs, 3 x LDS <= 160 KB); LDS exactly what the
    layouts add up to -- 400 bytes of line extensions in the cost kernels, 5G + 4 words per group in
    the block output.  The VGPR figures themselves are pinned in
    tests/test_kernel_resources.py."""
    mipgpu.library()
    want = {"angular_ext_kernel": 13708, "angular_ext_refine_kernel": 14012, "angular_ext_predict_kernel": 5376}
    for name, lds in want.items():
        k = _kernel(name)
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, name
        assert k[".group_segment_fixed_size"] == lds, name
    for name in ("angular_ext_kernel", "angular_ext_refine_kernel"):
        k = _kernel(name)
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 168 and 3 * k[".group_segment_fixed_size"] <= 160 * 1024
    plain = _kernel("angular_kernel")
    assert (plain[".group_segment_fixed_size"], plain[".private_segment_fixed_size"]) == (13308, 0)
    # the _ext kernels' names stay clear of the patterns other tests find their siblings by
    for name in kernel_resources.kernels(mipgpu.LIB_PATH):
        if "_ext_" in name:
            assert not re.search(r"\d+(angular_kernel|angular_refine_kernel|intra_kernel)E", name), name
            assert not any(part in name for part in ("filter_kernel", "mip_search_kernel", "candidates_kernel")), name


def test_dispatch_reads_the_setting_once_per_launch():
    with open(os.path.join(REPO, "vvc-mip-gpu_amd", "csrc", "host_stages.cpp")) as f:
        host = f.read()
    launch = host[host.index("static int predict_launch("):host.index("static int predict_args_ok(")]
    assert launch.count("e->ang_refs.load()") == 1 and "launch_predict_angular_ext(x, s)" in launch
    impl = host[host.index("static int angular_device_impl("):host.index("int mip_angular_device(")]
    assert impl.count("e->ang_refs.load()") == 1
    assert "launch_angular_ext_refine(a, s)" in impl and "launch_angular_ext(a, s)" in impl


# ---------------------------------------------------------------- non-vacuity of the GPU cases
def test_gpu_case_set_is_not_vacuous():
    """On the restatements alone, for the frames of tests/test_gpu_angular_ext.py: at least 10 % of
    the positive-angle entries of available CUs differ between extended and substituted tables;
    full, partial and zero lengths occur on both lines among the compared CUs; extensions are cut
    by the right and by the bottom frame edge; and with the engine filter of the GPU cases some CU's
    extension is cut by the filter's undefined set."""
    _, _, un, e_top, e_left, ext = XC.case(W, H)
    sub = XC.substituted(W, H)
    x, y, bw, bh = _geometry(W, H)
    slots = np.array(X.POSITIVE_MODES) - 2
    changed = (ext["cost"][:, ~un][:, :, slots] != sub["cost"][:, ~un][:, :, slots]).mean()
    assert changed >= 0.10, changed
    for e, full, name in ((e_top, bh, "top"), (e_left, bw, "left")):
        on = ~un
        assert (on & (e == full)).any() and (on & (e > 0) & (e < full)).any() and (on & (e == 0)).any(), name
    # cut by the frame's right edge / bottom edge: the next sample would be outside the frame,
    # although it precedes the CU in coding order
    right = ~un & (e_top < bh) & (y > 0) & (x + bw + e_top == W) & (x + bw <= W)
    bottom = ~un & (e_left < bw) & (x > 0) & (y + bh + e_left == H) & (x + bw <= W)
    assert right.any() and bottom.any()
    # both classes see changes, and the vertical class only through the top line
    assert (ext["cost"][:, :, 49:] != sub["cost"][:, :, 49:]).any() and (ext["cost"][:, :, :16] != sub["cost"][:, :, :16]).any()
    # the undefined set of a filter cuts an extension: the same availability set without the
    # undefined-sample condition gives a longer line somewhere
    cut = 0
    for filt in (XC.FILTER_2D, "filterFrame_1d_int"):
        un_f, top_f, left_f = XC.lengths(W, H, filt)
        und = XC.undefined(W, H, filt)
        assert und is not None and und.any(), filt
        free_top, free_left = X.lengths(W, H, un_f, None)
        cut += int(((free_top > top_f) | (free_left > left_f)).sum())
        assert np.all(free_top >= top_f) and np.all(free_left >= left_f)
    assert cut > 0
