"""Build-time resource checks of the gfx950 kernels in libmipgpu.so (CPU: reads the code
objects' metadata, tests/kernel_resources.py).

* No kernel spills to scratch (an out-of-line device helper in the search loop once cost
  192 bytes per lane of scratch, 12 % of the search time and 2x its HBM traffic) -- except the
  12-wave search kernels, which at 80 VGPRs keep up to 24 dwords of per-item state in scratch
  (item setup and window staging, once per quadrant item: none inside the size classes' code,
  tools/isa_dump.py); they are held to 96 bytes per lane.
* mip_search_kernel: the 12-wave variants <= 80 VGPRs, i.e. 6 waves per SIMD -- two 12-wave
  workgroups per CU; the 16-wave variants (small launches, one workgroup per CU) and the
  four-wave twin's 8-wave ones (the host pipeline's small chunks, two per CU) <= 128 VGPRs,
  4 waves per SIMD: the occupancy the persistent grid is sized for.
* filter_kernel: 2-D filters (128-thread tiles) <= 64 VGPRs, i.e. 8 waves per SIMD; the
  separable ones run one-wave 64-thread tiles (round 6) whose ~10 KB of LDS each allow 16 per
  CU, 4 waves per SIMD: <= 128 VGPRs.
* intra_kernel, the first of the kernels that cost every CU from a staged window and share
  their item walk and staging (csrc/mip_window_dev.h): <= 128 VGPRs, 4 waves per SIMD, no
  scratch.
* The angular family -- six cost kernels, four of them one body with a policy and two with the
  same walk as a body of their own (csrc/mip_angular.hip), three block outputs that are one body
  with a policy (csrc/mip_predict_angular.hip): no scratch, no spilled vector
  register; the cost kernels three waves per SIMD (at most 168 VGPRs, 3 x LDS <= 160 KB); LDS
  exactly what the layouts add up to; and the build's VGPR figures, pinned with equality in
  ANGULAR_FAMILY below, the one table of them (DESIGN.md section 5.7 has it beside the figures of
  the six separate bodies it replaced).  tests/test_angular_refine_cpu.py, test_angular_ext_cpu.py
  and test_angular_tap4_cpu.py hold their kernels to the same conditions by name.
"""
import os
import re

import pytest

import kernel_resources

LIB = os.path.join(os.path.dirname(__file__), "..", "vvc-mip-gpu_amd", "lib", "libmipgpu.so")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        pytest.skip("libmipgpu.so not built")
    return kernel_resources.kernels(LIB)


def _named(kernels, part):
    found = {n: k for n, k in kernels.items() if part in n}
    assert found, part
    return found


def test_every_kernel_variant_present(kernels):
    # {orig, alt} x {table, decisions} x prefetch (orig), and the 16-wave variants of small
    # launches ({orig, alt} x {table, decisions}, no prefetch)
    # + the four-wave twin's 8-wave variants ({orig, alt} x {table, decisions}, orig x prefetch)
    assert len(_named(kernels, "mip_search_kernel")) == 16
    assert len(_named(kernels, "filter_kernel")) == 8      # radius x int/float x 2-D/separable
    for part in ("fixup_kernel", "best_mode_kernel", "dec_split_kernel"):
        _named(kernels, part)


def _search_waves(name):
    return int(re.search(r"mip_search_kernelILb\dELb\dELb\dELi(\d+)EE", name).group(1))  # <ALT, DEC, PF, NW>


def test_no_scratch_spills(kernels):
    spilled = {n: k[".private_segment_fixed_size"] for n, k in kernels.items() if k[".private_segment_fixed_size"]}
    bounded = {n: b for n, b in spilled.items() if "mip_search_kernel" in n and _search_waves(n) == 12 and b <= 96}
    assert spilled == bounded, spilled


def test_search_kernel_occupancy(kernels):
    waves = set()
    for name, k in _named(kernels, "mip_search_kernel").items():
        nw = _search_waves(name)
        waves.add(nw)
        limit = 80 if nw == 12 else 128  # 6 / 4 waves per SIMD (8: the four-wave twin)
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= limit, (name, k[".vgpr_count"])
    assert waves == {8, 12, 16}


def test_filter_kernel_occupancy(kernels):
    for name, k in _named(kernels, "filter_kernel").items():
        sep = re.search(r"filter_kernelILi\dELb\dELb(\d)EE", name).group(1) == "1"  # <RAD, FLOAT, SEP>
        assert k[".vgpr_count"] <= (128 if sep else 64), (name, k[".vgpr_count"])


def test_intra_kernel_occupancy(kernels):
    found = {n: k for n, k in kernels.items() if re.search(r"\d+intra_kernelE", n)}
    assert len(found) == 1, found
    (name, k), = found.items()
    assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 128, (name, k[".vgpr_count"])
    assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, name


# kernel: (VGPRs, AGPRs included; LDS bytes).  LDS is the layout's: s_org 8192, s_ref 2256 (2656 with the
# two line extensions), s_sum 2080, s_tab 780; the refinement's s_pack 260 and s_cand 28 (and
# padding), the four taps' s_coef 256 -- an instantiation without one of them does not pay for it.
# Block output: 4 waves x 272 (336 with the extension) words, the four taps' 256 bytes.
# (angular_ext_kernel and angular_tap4_kernel keep a body of their own, and with it their earlier figures.)
ANGULAR_COST = {"angular_kernel": (124, 13308), "angular_refine_kernel": (131, 13612),
                "angular_ext_kernel": (133, 13708), "angular_ext_refine_kernel": (138, 14012),
                "angular_tap4_kernel": (147, 13968), "angular_tap4_refine_kernel": (147, 14268)}
ANGULAR_OUTPUT = {"angular_predict_kernel": (63, 4352), "angular_ext_predict_kernel": (78, 5376), "angular_tap4_predict_kernel": (78, 5632)}
ANGULAR_FAMILY = {**ANGULAR_COST, **ANGULAR_OUTPUT}


def test_angular_family_resources(kernels):
    got = {}
    for name in ANGULAR_FAMILY:
        found = [k for n, k in kernels.items() if re.search(r"\d+%sE" % name, n)]
        assert len(found) == 1, name
        k, = found
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, name
        got[name] = (k[".vgpr_count"] + k.get(".agpr_count", 0), k[".group_segment_fixed_size"])
    assert got == ANGULAR_FAMILY
    for name in ANGULAR_COST:
        assert got[name][0] <= 512 // 3 // 8 * 8 == 168 and 3 * got[name][1] <= 160 * 1024, name
    assert len([n for n in kernels if "angular" in n]) == len(ANGULAR_FAMILY)      # nine kernels, no stray instance
