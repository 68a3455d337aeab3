"""Shared, cached cases of the extended-reference angular tests (CPU and GPU) -- test helper, not
a test: the frames of tests/intra_cases.py at the GPU tests' size, their references, the
availability set, the two lengths per CU and the tables of the numpy restatement
(tests/angular_ext_ref.py), computed once per (size, reference source, frames, mode list); callers
do not modify the arrays."""
from functools import lru_cache

import numpy as np

import angular_ext_ref as X
import angular_ref as A
import intra_cases as C
import mipgpu
import oracle_lib as O
import size_sweep as S
from mipgpu import layout

SIZE = (264, 136)                                             # 3 x 2 CTUs, partial right column and bottom row
FILTER_2D = "filterFrame_2d_int_quarterCtu"                   # the engine filter of the GPU cases
TABLES = ("cost", "sad", "satd")
EVEN_MODES = tuple(range(2, 67, 2))
ODD_LENGTH_LIST = (2, 3, 10, 17, 18, 19, 34, 49, 50, 51, 58, 65, 66)      # 13 modes: the last round of two is half empty
BLOCK_MODES = (2, 10, 17, 18, 34, 50, 51, 58, 66)             # the block-output test's
SWEEP_LIST = (2, 9, 17, 18, 34, 50, 51, 59, 66)               # the frame-edge sweep's: both classes' positive angles, 18 / 34 / 50


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@lru_cache(maxsize=None)
def undefined(w, h, filt):
    """bool [H, W] or None: the samples the oracle's filter `filt` leaves undefined because it
    reads past the frame's end (bit 0 of its codes; the frame's content does not matter)."""
    if filt is None:
        return None
    _, und = O.filter_frame(np.zeros((h, w), np.uint16), filt, 0, with_undefined=True, kinds=True)
    return _freeze((und & 1).astype(bool))[0]


@lru_cache(maxsize=None)
def lengths(w, h, filt=None):
    """(availability set, E_top, E_left) of the restatement for an engine with filter `filt`."""
    un = mipgpu.unavailable_cus(w, h, filt)
    e_top, e_left = X.lengths(w, h, un, undefined(w, h, filt))
    return _freeze(un, e_top, e_left)


def length_class(e, full):
    """0: no extension, 1: a partial one, 2: the full one."""
    return np.where(e == 0, 0, np.where(e == full, 2, 1))


def length_class_cus(w, h, un, e_top, e_left, per=2):
    """The selector of the block-output tests: `per` CUs of every shape for each of the nine
    combinations of full / partial / zero lengths on the two lines that exists among the available
    CUs.  Sorted CU indexes."""
    shape, x, y, bw, bh = layout.cu_geometry(w, h, np.arange(un.size))
    kt, kl = length_class(e_top, bh), length_class(e_left, bw)
    picked = []
    for s in layout.SHAPES:
        for a in range(3):
            for b in range(3):
                k = np.nonzero(~un & (shape == s.index) & (kt == a) & (kl == b))[0]
                if k.size:
                    picked += list(k[np.unique(np.linspace(0, k.size - 1, per).astype(int))])
    return np.array(sorted(set(picked)), np.int64)


def _tables(f, refs, un, e_top, e_left, modes):
    ref = [X.tables(x, r, un, e_top, e_left, modes) for x, r in zip(f, refs)]
    tabs = {k: np.stack([t[k] for t in ref]) for k in TABLES}
    tabs["ang_mode"], tabs["ang_cost"] = A.best(tabs["cost"])
    _freeze(*tabs.values())
    return tabs


@lru_cache(maxsize=None)
def case(w, h, source=None, n=3, modes=None):
    """(frames [n, H, W], references, availability set, E_top, E_left, dict of the restatement's
    extended tables [n, nCTUs*5380, 65] plus 'ang_mode' / 'ang_cost').  source: None (the originals),
    a filter name (the oracle's filter; its availability and undefined-sample sets) or 'caller'
    (tests/size_sweep.py caller_refs per frame; the MIP_FILTER_NONE sets)."""
    f = C.frames(w, h, n)
    if source is None:
        refs = f
    elif source == "caller":
        refs = _freeze(np.stack([S.caller_refs(w, h, salt) for salt in range(n)]))[0]
    else:
        refs = _freeze(np.stack([O.filter_frame(x, source, 0) for x in f]))[0]
    un, e_top, e_left = lengths(w, h, source if source not in (None, "caller") else None)
    return f, refs, un, e_top, e_left, _tables(f, refs, un, e_top, e_left, modes)


@lru_cache(maxsize=None)
def substituted(w, h, source=None, n=3, modes=None):
    """The substituted tables (tests/angular_ref.py) of the same case."""
    f, refs, un, _, _, _ = case(w, h, source, n, modes)
    ref = [A.tables(x, r, un, modes) for x, r in zip(f, refs)]
    tabs = {k: np.stack([t[k] for t in ref]) for k in TABLES}
    tabs["ang_mode"], tabs["ang_cost"] = A.best(tabs["cost"])
    _freeze(*tabs.values())
    return tabs


def listed(tabs, modes):
    """The tables of the list `modes` out of 65-mode tables: the other slots UNAVAILABLE."""
    mask = np.zeros(A.MODES, bool)
    mask[np.array(modes) - A.FIRST] = True
    out = {k: np.where(mask, tabs[k], A.UNAVAILABLE).astype(np.int32) for k in TABLES}
    out["ang_mode"], out["ang_cost"] = A.best(out["cost"])
    return out


@lru_cache(maxsize=None)
def sweep_case(w, h, filt=None):
    """One `noise` frame of tests/size_sweep.py with SWEEP_LIST: (frame, refs, un, E_top, E_left, tables [ncu, 65] ...)."""
    frame = S.content("noise", w, h)
    refs = frame if filt is None else O.filter_frame(frame, filt, 0)
    un, e_top, e_left = lengths(w, h, filt)
    tabs = X.tables(frame, refs, un, e_top, e_left, SWEEP_LIST)
    tabs["ang_mode"], tabs["ang_cost"] = A.best(tabs["cost"])
    _freeze(frame, refs, *tabs.values())
    return frame, refs, un, e_top, e_left, tabs
