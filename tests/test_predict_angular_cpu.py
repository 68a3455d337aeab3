"""Angular block output on the CPU (no GPU): the write rule the prediction kernels share
(csrc/predict_rule.h), compiled stand-alone (tests/cpp/test_predict_rule.cpp, with
-fsanitize=address,undefined; no preloaded library) on arrays of exactly the sizes the rule may
index, equals a numpy restatement written from the contract text of include/mipgpu.h for every
flag combination; the same program checks the argument rules of the flags word and of
mip_predicted_frames_ex.  The constants the multi-pass GPU test is sized from
(tests/predict_angular_caps.py) are the shared launch's and the shared body's, read from their
text, and the three angular kernels and launchers are nothing but calls of those; the existing
launcher and kernel of mip_predict.hip keep exactly two instances of one kernel; and the Python
constants mirror the header."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mipgpu
import predict_angular_caps as L
from mipgpu import layout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the launcher's constants
def test_angular_predict_caps_are_the_launchers():
    with open(os.path.join(L.CSRC, L.SOURCE)) as f:
        text = f.read()
    assert "constexpr int kAngPredWaves = %d;" % L.WAVES in text
    assert "constexpr int kAngPredEntriesPerWave = %d;" % L.ENTRIES_PER_WAVE in text
    assert "constexpr int kAngPredGroupsCap = %d;" % L.GROUPS_CAP in text
    body = L.launcher_body(L.SOURCE, L.LAUNCH_RULE)                       # (to the end of the file: the three launchers too)
    assert "per_group = (long long)kAngPredWaves * kAngPredEntriesPerWave;" in body
    assert "groups = std::min<long long>((a.n + per_group - 1) / per_group, kAngPredGroupsCap);" in body
    assert body.count("dim3((unsigned)groups), dim3(64 * kAngPredWaves)") == 1 and text.count("hipLaunchKernelGGL(") == 1
    assert "cus" not in body and "multiProcessorCount" not in text       # the cap does not depend on the device
    for launcher, kernel, ext_ok in L.LAUNCHERS:                          # every launcher is a call of that launch with its kernel
        assert "return %s(%s, a, %s, s);" % (L.LAUNCH_RULE, kernel, ext_ok) in L.launcher_function(L.SOURCE, launcher), launcher
        assert L.wrapped_body(L.SOURCE, kernel) == L.BODY, kernel         # and every kernel nothing but a call of the one body
    kernel = L.kernel_body(L.SOURCE, L.KERNEL)
    assert kernel.startswith("void %s(" % L.BODY)
    assert "rows = (a.n + kAngPredEntriesPerWave - 1) / kAngPredEntriesPerWave;" in kernel
    assert "r = (long long)blockIdx.x * kAngPredWaves + wv; r < rows; r += (long long)gridDim.x * kAngPredWaves" in kernel
    assert "idx = r * kAngPredEntriesPerWave + lane;" in kernel and "lane = threadIdx.x & 63" in kernel
    assert text.count("atomicSub(a.skipped") == 1 == kernel.count("atomicSub(a.skipped")      # one list scan in the block-output sources
    for once in ("Item take_item(", "void store_angular(", "void predict_angular_cu(", "void wave_lds_sync("):
        assert text.count(once) == 1, once
    # wave-private LDS: no workgroup barrier in the scan -- the only one stands before it, behind the 4-tap coefficients' staging
    assert text.count("__syncthreads()") == 1 == kernel.count("__syncthreads()")
    assert kernel.index("s_coef[threadIdx.x] = a.coef[threadIdx.x];") < kernel.index("__syncthreads()") < kernel.index("for (long long r =")
    assert L.ENTRIES_PER_WAVE == 64                                       # one entry per lane of a wave
    assert L.ENTRIES_PER_ROUND == L.GROUPS_CAP * L.WAVES * L.ENTRIES_PER_WAVE == 262144
    assert L.ROWS_PER_ROUND * L.ENTRIES_PER_WAVE == L.ENTRIES_PER_ROUND
    work = L.multipass_work(L.ENTRIES_PER_ROUND)
    assert work == 611669 and work < 1 << 20                              # the multi-pass list stays below a million entries
    assert L.passes(-(-work // (L.WAVES * L.ENTRIES_PER_WAVE)), L.GROUPS_CAP) == (2, 3)


def test_the_mip_kernel_and_its_launcher_are_left_alone():
    """The angular kernels are a file and launchers of their own: launch_predict still launches two
    instances of predict_kernel and nothing else, and the shared rule is the one function both
    files' kernels call."""
    body = L.launcher_body("mip_predict.hip", "launch_predict")
    assert body.count("hipLaunchKernelGGL(") == 2 and "angular" not in body
    with open(os.path.join(L.CSRC, "mip_predict.hip")) as f:
        mip = f.read()
    with open(os.path.join(L.CSRC, L.SOURCE)) as f:
        ang = f.read()
    assert "pred_decode<REGULAR, false>(a, it, PredShapes{})" in mip and "pred_decode<false, true>(a, it, AngShapes{})" in ang
    for text in (mip, ang):
        assert '#include "predict_rule.h"' in text and "it.pitch <" not in text    # no copy of the rule
    with open(os.path.join(L.CSRC, "host_stages.cpp")) as f:
        host = f.read()
    launch = host[host.index("static int predict_launch("):host.index("static int predict_args_ok(")]
    assert launch.index("launch_predict(a, s)") < launch.index("if (flags & MIP_PRED_ANGULAR)") < launch.index("launch_predict_angular(a, s)")


def test_python_constants_mirror_the_header():
    src = open(os.path.join(REPO, "include", "mipgpu.h")).read()
    defs = {k: int(v.rstrip("uU"), 0) for k, v in re.findall(r"^#define\s+(MIP_\w+)\s+(0x[0-9a-fA-F]+|\d+)[uU]?\b", src, flags=re.M)}
    assert defs["MIP_PRED_ANGULAR"] == mipgpu.PRED_ANGULAR == 4 and defs["MIP_PRED_REGULAR"] == mipgpu.PRED_REGULAR == 1
    assert defs["MIP_CHAIN_ANGULAR"] == mipgpu.CHAIN_ANGULAR == 1
    assert re.search(r"^#define\s+MIPGPU_ABI_VERSION\s+7$", src, flags=re.M)   # additive: the ABI version stays
    assert "PRED_ANGULAR" in mipgpu.__all__ and "CHAIN_ANGULAR" in mipgpu.__all__
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert ("const int32_t *penalty, const int32_t *bias, const uint8_t *ang_modes, int ang_nmodes, int32_t ang_bias, "
            "unsigned flags, uint8_t *best_mode_out,") in text
    sig = inspect.signature
    assert sig(mipgpu.MipEngine.predict).parameters["angular"].default is False
    assert sig(mipgpu.MipEngine.predict_device).parameters["angular"].default is False
    p = sig(mipgpu.MipEngine.predicted_frames_ex).parameters
    assert list(p) == ["self", "frames", "penalty", "bias", "refs", "angular", "angular_bias"]
    assert p["angular"].default is None and p["angular_bias"].default == 0
    lib = mipgpu.library()
    assert lib.mip_abi_version() == 7
    assert lib.mip_predicted_frames_ex(None, None, None, 1, None, None, None, 0, 0, 0, None, None, None, None, None, None) != 0
    assert b"engine is NULL" in lib.mip_last_error()


# ---------------------------------------------------------------- the shared write rule
@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("predict_rule") / "test_predict_rule"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "vvc-mip-gpu_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", str(exe),
                           os.path.join(REPO, "tests", "cpp", "test_predict_rule.cpp")])
    return str(exe)


def test_argument_rules(rule_exe):
    r = subprocess.run([rule_exe, "self"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "predict_rule: ok\n", (r.returncode, r.stdout + r.stderr)


def write_rule(w, h, nframes, out_samples, unavailable, items, regular, angular):
    """The write rule of include/mipgpu.h, item by item, from the contract text: (on, reg, x, y,
    bw, bh) int32 [n, 6], zeros behind on = 0."""
    ncu = unavailable.size
    out = np.zeros((items.size, 6), np.int32)
    for i, it in enumerate(items):
        frame, cu, mode, pitch, offset = (int(it[k]) for k in ("frame", "cu", "mode", "pitch", "offset"))
        if not (0 <= frame < nframes and 0 <= cu < ncu) or unavailable[cu]:
            continue
        shape, x, y, bw, bh = (int(v[0]) for v in layout.cu_geometry(w, h, [cu]))
        reg = regular and mode in (mipgpu.MODE_PLANAR, mipgpu.MODE_DC)
        ang = angular and mipgpu.MODE_ANGULAR_BASE + 2 <= mode <= mipgpu.MODE_ANGULAR_BASE + 66
        if not (reg or ang or 0 <= mode < layout.SHAPES[shape].total_modes):
            continue
        if pitch < bw or pitch % 4 or offset % 4 or offset < 0 or offset + (bh - 1) * pitch + bw > out_samples:
            continue
        out[i] = (1, reg, x, y, bw, bh)
    return out


def test_rule_equals_the_contract_for_every_flag_combination(rule_exe, tmp_path):
    """264x136, two frames: items of every shape with MIP, Planar, DC and angular modes (both ends
    of the code range and the codes next to it), and every kind of rejected entry -- among them
    indexes far outside the tables, which the exactly-sized arrays turn into a sanitizer report
    if the rule reads before it checks."""
    w, h, nframes = 264, 136, 2
    un = mipgpu.unavailable_cus(w, h)
    rng = np.random.default_rng(0xA9)
    ok = np.nonzero(~un)[0]
    cus = np.concatenate([rng.choice(ok, 1200), rng.choice(np.nonzero(un)[0], 60)])
    modes = rng.choice(np.array([0, 1, 5, 11, 12, 15, 16, 31, 32, -1, 0x7F, 0x80, 0x81, 0x82, 0x83, 0x92, 0xA2, 0xB2, 0xC1, 0xC2,
                                 0xC3, 0xEF, 0xF0, 0xF1, 0xF2, 0xFF, 0x100 + 0x82, 1 << 30]), cus.size)
    items, total = mipgpu.pred_items(w, h, rng.integers(0, nframes, cus.size), cus, modes, nframes=nframes)
    n = items.size
    kind = rng.integers(0, 28, n)                            # (kinds 11 and up: the item as laid out)
    bw = layout.cu_geometry(w, h, cus)[3]
    items["frame"][kind == 0] = rng.choice([-1, nframes, 1 << 30, -(1 << 31)], int((kind == 0).sum()))
    items["cu"][kind == 1] = rng.choice([-1, un.size, un.size + 5380, (1 << 31) - 1, -(1 << 31)], int((kind == 1).sum()))
    items["pitch"][kind == 2] = bw[kind == 2] - 4
    items["pitch"][kind == 3] += 2
    items["offset"][kind == 4] += 2
    items["offset"][kind == 5] = -4
    items["offset"][kind == 6] = total - 4                    # starts inside out_samples, ends past it
    items["offset"][kind == 7] = (1 << 62)
    items["pitch"][kind == 8] = (1 << 31) - 4                 # (h - 1) * pitch needs 64 bits
    fits = total - (layout.cu_geometry(w, h, cus)[4] * bw)    # the last block that still fits, at pitch = w
    items["offset"][kind == 9] = fits[kind == 9]
    items["offset"][kind == 10] = fits[kind == 10] + 4        # one row of four too far
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([w, h, nframes, n], np.int32).tobytes() + np.array([total], np.int64).tobytes())
        f.write(un.astype(np.uint8).tobytes() + items.tobytes())
    r = subprocess.run([rule_exe, "decode", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "predict_rule: decoded %d items\n" % n, (r.returncode, r.stdout + r.stderr)
    got = np.fromfile(dst, np.int32).reshape(4, n, 6)
    seen = []
    for q, (regular, angular) in enumerate(((False, False), (True, False), (False, True), (True, True))):
        want = write_rule(w, h, nframes, total, un, items, regular, angular)
        bad = np.nonzero((got[q] != want).any(axis=1))[0]
        assert bad.size == 0, (regular, angular, bad[:4], items[bad[:4]], got[q][bad[:4]], want[bad[:4]])
        seen.append(want[:, 0].astype(bool))
    none, reg, ang, both = seen
    is_ang = (items["mode"] >= 0x82) & (items["mode"] <= 0xC2)
    is_reg = (items["mode"] == 0xF0) | (items["mode"] == 0xF1)
    assert none.any() and not (none & (is_ang | is_reg)).any()               # flags 0: MIP items only
    assert np.array_equal(reg & ~is_reg, none) and np.array_equal(ang & ~is_ang, none)
    assert np.array_equal(both, reg | ang) and not (reg & ang & ~none).any()
    assert (ang & is_ang).sum() > 20 and (reg & is_reg).sum() > 5
    for code in (0x82, 0xC2):                                               # both ends of the range are emitted ...
        assert (ang & (items["mode"] == code)).any()
    for code in (0x80, 0x81, 0xC3, 0xFF, 0x182):                            # ... and the codes around it never
        assert (items["mode"] == code).any() and not (both & (items["mode"] == code)).any()
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10):                               # every rejected kind is in the list and is rejected
        assert (kind == k).any() and not both[kind == k].any(), k
    assert both[kind == 9].any()                                            # the last block that fits is written
