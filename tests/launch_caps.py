"""Grid caps of the grid-stride kernels -- a helper, not a test.  The partition, intra and
prediction kernels reuse their LDS arrays from one pass to the next; the copy kernel has a main
loop and a tail loop that split the work of a pass.  tests/test_gpu_multipass.py,
tests/test_gpu_predict_multipass.py and tests/test_gpu_copy.py size their work from these
factors so that every workgroup runs at least two passes; the CPU test of
tests/test_gpu_multipass.py reads the launchers' text and fails when a factor here no longer
is the launcher's.  The intra kernel and the six angular cost kernels have one item walk, one
window staging and one launch rule between them, in WINDOW_HEADER: window_text() is that file, and
uses_window_rules() says whether a launcher and the code its kernel runs go through it.  The nine
angular kernels (six cost kernels, three block outputs) are one-line wrappers of a shared body:
kernel_body() follows a wrapper to the body it calls, wrapped_body() names that body.

  launch_partition (vvc-mip-gpu_amd/csrc/mip_partition.hip): grid = min(groups, 8 * CUs),
      groups = frames * CTUs, one (frame, CTU) pair per pass;
  launch_intra (vvc-mip-gpu_amd/csrc/mip_intra.hip), through launch_window_kernel
      (vvc-mip-gpu_amd/csrc/mip_window_dev.h): grid = min(items, 32 * CUs),
      items = frames * CTUs * 20 -- per CTU the four 64x64 CUs, then the sixteen 32x32 blocks.
  launch_predict (vvc-mip-gpu_amd/csrc/mip_predict.hip): grid = min(ceil(n / 16), 256 * 16)
      workgroups of 4 waves, a wave takes 4 consecutive list items per pass (one per 16 lanes):
      one round of the capped grid is 65 536 items, independent of the CU count;
  launch_copy (vvc-mip-gpu_amd/csrc/mip_filter.hip): grid = min(ceil(n16 / 1024), 8 * CUs)
      workgroups of 256 lanes, 1024 uint4 per workgroup and iteration: four per lane while
      `i + 768 < n16`, then one per lane in the tail loop.
"""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "vvc-mip-gpu_amd", "csrc")

PARTITION_GROUPS_PER_CU = 8
INTRA_ITEMS_PER_CU = 32
INTRA_ITEMS_PER_CTU = 20        # kItemsPerCtu = 4 + kIntraBlocks
INTRA_BIG_ITEMS = 4             # items k < 4 of a CTU are its 64x64 CUs

PREDICT_GROUPS_CAP = 256 * 16    # workgroups, whatever the device
PREDICT_WAVES = 4               # kPredWaves
PREDICT_ITEMS_PER_WAVE = 4      # kPredItemsPerWave
PREDICT_ITEMS_PER_ROUND = PREDICT_GROUPS_CAP * PREDICT_WAVES * PREDICT_ITEMS_PER_WAVE   # 65 536
PREDICT_QUADS_PER_ROUND = PREDICT_GROUPS_CAP * PREDICT_WAVES    # a wave's passes are quads q, q + 16 384, ...

COPY_GROUPS_PER_CU = 8
COPY_WORDS_PER_GROUP = 1024     # uint4 per workgroup and iteration
COPY_MAIN_LOOP_REACH = 768      # the main loop runs while i + 768 < n16

# (source file, function that holds the cap, factor): the cap reads `groups < F * cus ? groups : F * cus`
WINDOW_HEADER = "mip_window_dev.h"
LAUNCHERS = (
    ("mip_partition.hip", "launch_partition", PARTITION_GROUPS_PER_CU),
    (WINDOW_HEADER, "launch_window_kernel", INTRA_ITEMS_PER_CU),
)
CAP_EXPRESSION = re.compile(r"grid\s*=\s*groups\s*<\s*(\d+)LL\s*\*\s*cus\s*\?\s*groups\s*:\s*(\d+)LL\s*\*\s*cus\s*;")


def launcher_body(source, launcher):
    """The text of `launcher` in csrc/`source`, from its signature to the end of the file's namespace."""
    with open(os.path.join(CSRC, source)) as f:
        text = f.read()
    at = text.index("hipError_t %s(" % launcher)
    return text[at:]


def window_text():
    """The header of the intra and angular kernels' shared item walk, staging and launch rules."""
    with open(os.path.join(CSRC, WINDOW_HEADER)) as f:
        return f.read()


def uses_window_rules(source, launcher, kernel):
    """`launcher` takes its argument and grid rules, the code of `kernel` its items and staging, from WINDOW_HEADER."""
    body, code = launcher_function(source, launcher), kernel_body(source, kernel)
    return ("window_args_ok(a)" in body and "return launch_window_kernel(%s, a, s);" % kernel in body and "hipLaunchKernelGGL" not in body
            and "window_item(g, a.nctus, a.ctu_cols, frame_samples, a.orig, a.refs)" in code and "stage_window(it.F, it.R, a.width," in code)


def launcher_function(source, launcher):
    """The text of `launcher` alone, from its signature to the closing brace of its body."""
    text = launcher_body(source, launcher)
    return text[:text.index("\n}\n")]


WRAPPER = r"__global__ [^;{}]*\bvoid %s\(\w+ a\) \{ (\w+)<[\w, ]+>\(a\); \}\n"


def wrapped_body(source, kernel):
    """The shared body that `kernel` is a one-line wrapper of (nothing but its call, the kernel's
    argument struct handed on as it is), or None where the kernel has a body of its own."""
    with open(os.path.join(CSRC, source)) as f:
        m = re.search(WRAPPER % kernel, f.read())
    return m.group(1) if m else None


def kernel_body(source, kernel):
    """The text of the code `kernel` runs in csrc/`source`: its own body from its name to the closing
    brace, or that of the shared body it wraps."""
    with open(os.path.join(CSRC, source)) as f:
        text = f.read()
    at = text.index("void %s(" % (wrapped_body(source, kernel) or kernel))
    return text[at:text.index("\n}\n", at)]


def partition_cap(cus):
    return PARTITION_GROUPS_PER_CU * cus


def intra_cap(cus):
    return INTRA_ITEMS_PER_CU * cus


def copy_cap(cus):
    return COPY_GROUPS_PER_CU * cus


def multipass_work(cap):
    """Work of a multi-pass batch: two full rounds of the capped grid and a third of a round."""
    return 2 * cap + cap // 3


def passes(work, cap):
    """(fewest, most) passes of a workgroup of a grid of min(work, cap) over `work` items."""
    grid = min(work, cap)
    return work // grid, -(-work // grid)
