"""The host pipeline's policy (vvc-mip-gpu_amd/csrc/host_policy.h: call signature, merge
decision, chunk sizes) on CPU: a C++ unit test built with g++ (no GPU), once plain and once
under AddressSanitizer / UndefinedBehaviorSanitizer; each is a stand-alone program."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_host_policy(tmp_path, flags):
    exe = tmp_path / "test_host_policy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I",
                           os.path.join(REPO, "vvc-mip-gpu_amd", "csrc"), "-o", str(exe),
                           os.path.join(REPO, "tests", "cpp", "test_host_policy.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_policy: ok" in r.stdout
