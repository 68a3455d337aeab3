"""Grid caps of the two grid-stride kernels whose workgroups reuse their LDS arrays from one
pass to the next -- a helper, not a test.  tests/test_gpu_multipass.py sizes its batches from
these factors so that every workgroup runs at least two passes; its CPU test reads the
launchers' text and fails when a factor here no longer is the launcher's.

  launch_partition (vvc-mip-gpu_amd/csrc/mip_partition.hip): grid = min(groups, 8 * CUs),
      groups = frames * CTUs, one (frame, CTU) pair per pass;
  launch_intra (vvc-mip-gpu_amd/csrc/mip_intra.hip): grid = min(items, 32 * CUs),
      items = frames * CTUs * 20 -- per CTU the four 64x64 CUs, then the sixteen 32x32 blocks.
"""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "vvc-mip-gpu_amd", "csrc")

PARTITION_GROUPS_PER_CU = 8
INTRA_ITEMS_PER_CU = 32
INTRA_ITEMS_PER_CTU = 20        # kItemsPerCtu = 4 + kIntraBlocks
INTRA_BIG_ITEMS = 4             # items k < 4 of a CTU are its 64x64 CUs

# (source file, launcher, factor): the launcher's cap reads `groups < F * cus ? groups : F * cus`
LAUNCHERS = (
    ("mip_partition.hip", "launch_partition", PARTITION_GROUPS_PER_CU),
    ("mip_intra.hip", "launch_intra", INTRA_ITEMS_PER_CU),
)
CAP_EXPRESSION = re.compile(r"grid\s*=\s*groups\s*<\s*(\d+)LL\s*\*\s*cus\s*\?\s*groups\s*:\s*(\d+)LL\s*\*\s*cus\s*;")


def launcher_body(source, launcher):
    """The text of `launcher` in csrc/`source`, from its signature to the end of the file's namespace."""
    with open(os.path.join(CSRC, source)) as f:
        text = f.read()
    at = text.index("hipError_t %s(" % launcher)
    return text[at:]


def partition_cap(cus):
    return PARTITION_GROUPS_PER_CU * cus


def intra_cap(cus):
    return INTRA_ITEMS_PER_CU * cus


def multipass_work(cap):
    """Work of a multi-pass batch: two full rounds of the capped grid and a third of a round."""
    return 2 * cap + cap // 3


def passes(work, cap):
    """(fewest, most) passes of a workgroup of a grid of min(work, cap) over `work` items."""
    grid = min(work, cap)
    return work // grid, -(-work // grid)
