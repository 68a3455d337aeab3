"""The search work planner (vvc-mip-gpu_amd/csrc/work_plan.h: MFMA tables, CTU variants, wave
tasks and their lists, the item order, the choice among the lists) on CPU: a C++ unit test
(tests/cpp/test_work_plan.cpp) that compares digests of every array an engine uploads with
constants recorded before the planner left mipgpu.cpp, and asserts the lists' structure.  Built
with g++ and with the ROCm clang++ (the library's host compiler): both must agree on every
digest, since the lists go through double costs, std::ceil and stable_sort."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")


def _run(compiler, opt, tmp_path):
    exe = tmp_path / "test_work_plan"
    subprocess.check_call([compiler, "-std=c++17", opt, "-Wall", "-Werror",
                           "-I", os.path.join(REPO, "vvc-mip-gpu_amd", "csrc"), "-I", os.path.join(REPO, "include"),
                           "-o", str(exe), os.path.join(REPO, "tests", "cpp", "test_work_plan.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "work_plan: ok" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_work_plan(tmp_path):
    _run("g++", "-O1", tmp_path)


@pytest.mark.skipif(not os.path.exists(ROCM_CLANG), reason="needs the ROCm clang++")
def test_work_plan_rocm_clang(tmp_path):
    _run(ROCM_CLANG, "-O3", tmp_path)
