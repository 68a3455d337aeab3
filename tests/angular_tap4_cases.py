"""Shared, cached cases of the 4-tap angular tests (CPU and GPU) -- test helper, not a test: the
frames, references, availability set and lengths of tests/angular_ext_cases.py with the tables of
the 4-tap restatement (tests/angular_tap4_ref.py), under either reference setting, computed once
per (size, setting, reference source, frames, mode list); callers do not modify the arrays."""
from functools import lru_cache

import numpy as np

import angular_ext_cases as XC
import angular_ref as A
import angular_tap4_ref as T
import oracle_lib as O
import size_sweep as S

SIZE = XC.SIZE                                                # 264x136: 3 x 2 CTUs, partial right column and bottom row
TABLES = XC.TABLES
EXT, SUB = 1, 0                                               # MIP_ANG_REFS_EXTENDED / _SUBSTITUTED
EVEN_MODES = XC.EVEN_MODES
# 15 modes: both classes, the angles +-1 next to both pure modes, both ends, 34, and a half-empty last round of two
ODD_LENGTH_LIST = (2, 3, 9, 17, 18, 19, 33, 34, 35, 49, 50, 51, 59, 65, 66)
BLOCK_MODES = (2, 9, 17, 18, 19, 34, 49, 50, 51, 59, 66)      # the block-output test's
SWEEP_LIST = (2, 9, 17, 18, 19, 34, 35, 50, 51, 59, 66)       # the frame-edge sweep's


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _lengths(refs_setting, e_top, e_left):
    if refs_setting == EXT:
        return e_top, e_left
    return _freeze(np.zeros_like(e_top), np.zeros_like(e_left))


def _tables(f, refs, un, e_top, e_left, modes):
    ref = [T.tables(x, r, un, e_top, e_left, modes) for x, r in zip(f, refs)]
    tabs = {k: np.stack([t[k] for t in ref]) for k in TABLES}
    tabs["ang_mode"], tabs["ang_cost"] = A.best(tabs["cost"])
    _freeze(*tabs.values())
    return tabs


@lru_cache(maxsize=None)
def inputs(w, h, source=None, n=3):
    """(frames [n, H, W], references, availability set, E_top, E_left) of angular_ext_cases.case
    without its tables.  source: None (the originals), a filter name or 'caller'."""
    f = XC.C.frames(w, h, n)
    if source is None:
        refs = f
    elif source == "caller":
        refs = _freeze(np.stack([S.caller_refs(w, h, salt) for salt in range(n)]))[0]
    else:
        refs = _freeze(np.stack([O.filter_frame(x, source, 0) for x in f]))[0]
    un, e_top, e_left = XC.lengths(w, h, source if source not in (None, "caller") else None)
    return f, refs, un, e_top, e_left


@lru_cache(maxsize=None)
def case(w, h, refs_setting=EXT, source=None, n=3, modes=None):
    """(frames, references, availability set, E_top, E_left as the setting gives them -- zeros under
    SUB --, dict of the 4-tap restatement's tables [n, nCTUs*5380, 65] plus 'ang_mode' / 'ang_cost')."""
    f, refs, un, e_top, e_left = inputs(w, h, source, n)
    e_top, e_left = _lengths(refs_setting, e_top, e_left)
    return f, refs, un, e_top, e_left, _tables(f, refs, un, e_top, e_left, modes)


listed = XC.listed


@lru_cache(maxsize=None)
def sweep_case(w, h, refs_setting=EXT, modes=None):
    """One `noise` frame of tests/size_sweep.py with the list `modes` (None: all 65):
    (frame, un, E_top, E_left, tables [ncu, 65] ...)."""
    frame = S.content("noise", w, h)
    un, e_top, e_left = XC.lengths(w, h, None)
    e_top, e_left = _lengths(refs_setting, e_top, e_left)
    tabs = T.tables(frame, frame, un, e_top, e_left, modes)
    tabs["ang_mode"], tabs["ang_cost"] = A.best(tabs["cost"])
    _freeze(frame, *tabs.values())
    return frame, un, e_top, e_left, tabs
