"""Planar / DC baseline costs on the CPU (no GPU): the host walk of csrc/intra_plan.h -- the
per-4x4-block arithmetic the kernel runs one lane per block -- compiled stand-alone
(tests/cpp/test_intra_plan.cpp, with -fsanitize=address,undefined; no preloaded library)
equals the numpy restatement tests/intra_ref.py bit for bit in every table and in the merge,
on structured, noise and 0 / 1023 frames at 136x72 and 60x36; the same program checks the
kernel's lane-slot lists against the shape table."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import intra_cases as C
import intra_ref as I
from mipgpu import layout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER = C.FILTER

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("intra_plan") / "test_intra_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "vvc-mip-gpu_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", str(exe),
                           os.path.join(REPO, "tests", "cpp", "test_intra_plan.cpp")])
    return str(exe)


def run_plan(exe, tmp_path, frames, refs, unavailable, best_mode, best_cost, bias):
    nf, h, w = frames.shape
    ncu = unavailable.size
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([w, h, nf, bias[0], bias[1]], np.int32).tobytes())
        for a, dt in ((frames, np.uint16), (refs, np.uint16), (unavailable, np.uint8), (best_mode, np.uint8), (best_cost, np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "intra_plan: ok" in r.stdout, (r.returncode, r.stdout + r.stderr)
    raw = open(dst, "rb").read()
    out, at = {}, 0
    for key, dt, count, shape in (("cost", np.int32, nf * ncu * 2, (nf, ncu, 2)), ("sad", np.int32, nf * ncu * 2, (nf, ncu, 2)),
                                  ("satd", np.int32, nf * ncu * 2, (nf, ncu, 2)), ("best_mode", np.uint8, nf * ncu, (nf, ncu)),
                                  ("best_cost", np.int32, nf * ncu, (nf, ncu))):
        out[key] = np.frombuffer(raw, dt, count, at).reshape(shape)
        at += count * np.dtype(dt).itemsize
    assert at == len(raw)
    return out


@pytest.mark.parametrize("filt", (None, FILTER), ids=("orig", "1d_int"))
@pytest.mark.parametrize("size", ((136, 72), (60, 36)), ids=lambda s: "%dx%d" % s)
def test_host_walk_equals_the_restatement(plan_exe, tmp_path, size, filt):
    w, h = size
    frames, refs, un, ref = C.case(w, h, filt)
    assert un.any() and not un.all()
    if filt is not None and w % 128:
        assert refs.max() > 1023                              # the only way the clip can fire
    rng = np.random.default_rng(w)
    # MIP decisions for the merge: around the Planar / DC costs, with exact ties and unavailable CUs
    avail_cost = np.where(ref["cost"] == layout.UNAVAILABLE, 0, ref["cost"]).min(axis=2)
    best_cost = (avail_cost + rng.integers(-40, 41, avail_cost.shape) * rng.integers(0, 2, avail_cost.shape)).clip(0).astype(np.int32)
    best_mode = rng.integers(0, 12, best_cost.shape).astype(np.uint8)
    dead = np.broadcast_to(un, best_cost.shape) | (rng.random(best_cost.shape) < 0.05)
    best_cost[dead], best_mode[dead] = layout.UNAVAILABLE, 0xFF
    for bias in ((0, 0), (7, 3)):
        got = run_plan(plan_exe, tmp_path, frames, refs, un, best_mode, best_cost, bias)
        for key in ("cost", "sad", "satd"):
            assert np.array_equal(got[key], ref[key]), key
        assert np.array_equal(got["cost"][:, :, 0] == layout.UNAVAILABLE, np.broadcast_to(un, best_cost.shape))
        mode, cost = I.merge(best_mode, best_cost, ref["cost"], bias)
        assert np.array_equal(got["best_mode"], mode) and np.array_equal(got["best_cost"], cost)
        assert (mode == I.MODE_PLANAR).any() and (mode == I.MODE_DC).any() and (mode < 12).any()
        assert np.array_equal(mode[dead], best_mode[dead])    # unavailable CUs stay as they are
