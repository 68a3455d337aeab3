"""The hardware facts phase A's clipping conversion rests on (mip_search.hip convert_pair):
bin/pknorm_probe (tools/pknorm_probe.hip, built by the engine's Makefile) on the GPU -- the
conversion over every value (D + beta) / 1024 of its grid and the MFMA's exactness with the
scaled operands.  One child process, one launch over 16.7 M values and six small ones."""
import os
import re
import subprocess

import pytest

from test_phase_a_convert_cpu import _kernel_beta

PROBE = os.path.join(os.path.dirname(__file__), "..", "vvc-mip-gpu_amd", "bin", "pknorm_probe")


@pytest.mark.gpu
def test_pknorm_probe(gpu_available):
    assert os.path.exists(PROBE), "bin/pknorm_probe is not built"
    r = subprocess.run([PROBE], capture_output=True, text=True, timeout=120)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    log2 = {2.0 ** -7: 7, 2.0 ** -6: 6}[_kernel_beta()]
    m = re.search(r"^convert beta=2\^-%d: (\d+) mismatches over the kernel's values" % log2, r.stdout, re.M)
    assert m and int(m.group(1)) == 0, r.stdout
    mfma = re.findall(r"^mfma beta=2\^-%d sizeId (\d): (\d+) of \d+ \(K rows 0\.\.7\) and (\d+) of \d+" % log2, r.stdout, re.M)
    assert sorted(int(s) for s, _, _ in mfma) == [0, 1, 2], r.stdout
    assert all(int(a) == 0 and int(b) == 0 for _, a, b in mfma), r.stdout
    assert "verdict: beta=2^-%d is exact" % log2 in r.stdout
