"""Shared, cached cases of the angular intra-cost tests (CPU and GPU) -- test helper, not a test:
the frames of tests/intra_cases.py (structured, noise, samples 0 / 1023 only), their references,
the availability set and the tables of the numpy restatement (tests/angular_ref.py), computed
once per (size, filter, frames, mode list); and the grid cap of launch_angular for the
multi-pass test."""
from functools import lru_cache

import numpy as np

import angular_ref as A
import intra_cases as C
import launch_caps
import mipgpu
import oracle_lib as O

FILTER = C.FILTER
TABLES = ("cost", "sad", "satd")
EVEN_MODES = tuple(range(2, 67, 2))

# The six angular cost launchers (vvc-mip-gpu_amd/csrc/mip_angular.hip) go through
# launch_window_kernel (vvc-mip-gpu_amd/csrc/mip_window_dev.h): grid = min(items, 32 * CUs) over the
# intra kernel's items -- frames * CTUs * 20, per CTU the four 64x64 CUs, then the sixteen 32x32
# blocks.  tests/test_angular_cpu.py compares the factor with that function's text.
ANGULAR_ITEMS_PER_CU = 32
ANGULAR_ITEMS_PER_CTU = launch_caps.INTRA_ITEMS_PER_CTU
ANGULAR_BIG_ITEMS = launch_caps.INTRA_BIG_ITEMS
# (launcher, kernel) of that file.  A kernel is a one-line wrapper of COST_BODY, except the two of
# COST_OWN_BODY, which keep the same walk as a body of their own because they were measured slower
# as instances of it (tests/test_angular_refine_cpu.py reads the text).
COST_SOURCE = "mip_angular.hip"
COST_BODY = "angular_items"
COST_OWN_BODY = ("angular_ext_kernel", "angular_tap4_kernel")
COST_KERNELS = (("launch_angular", "angular_kernel"), ("launch_angular_refine", "angular_refine_kernel"),
                ("launch_angular_ext", "angular_ext_kernel"), ("launch_angular_ext_refine", "angular_ext_refine_kernel"),
                ("launch_angular_tap4", "angular_tap4_kernel"), ("launch_angular_tap4_refine", "angular_tap4_refine_kernel"))


def angular_cap(cus):
    return ANGULAR_ITEMS_PER_CU * cus


def structured(kind, w, h, seed=0x3C1):
    """A frame whose sample at (x, y) is f(x), f(y) or f(x - y), f a table of random 10-bit
    values (non-periodic)."""
    f = np.random.default_rng(seed).integers(0, 1024, w + h + 1)
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    t = {"x": x + 0 * y, "y": y + 0 * x, "x-y": x - y + h}[kind]
    return f[t].astype(np.uint16)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@lru_cache(maxsize=None)
def references(w, h, filt, n=3):
    f = C.frames(w, h, n)
    return f if filt is None else _freeze(np.stack([O.filter_frame(x, filt, 0) for x in f]))[0]


@lru_cache(maxsize=None)
def case(w, h, filt, n=3, modes=None):
    """(frames [n, H, W], references (the oracle's filter `filt`, or the originals), the
    availability set, dict of the restatement's tables [n, nCTUs*5380, 65] plus its best angular
    modes 'ang_mode' / 'ang_cost' [n, nCTUs*5380]) for the mode list `modes` (a tuple; None: all)."""
    f, refs = C.frames(w, h, n), references(w, h, filt, n)
    un = mipgpu.unavailable_cus(w, h, filt)
    ref = [A.tables(x, r, un, modes) for x, r in zip(f, refs)]
    tabs = {k: np.stack([t[k] for t in ref]) for k in TABLES}
    tabs["ang_mode"], tabs["ang_cost"] = A.best(tabs["cost"])
    _freeze(un, *tabs.values())
    return f, refs, un, tabs
