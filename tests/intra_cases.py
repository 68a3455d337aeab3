"""Shared, cached cases of the Planar / DC baseline-cost tests (CPU and GPU) -- test helper, not
a test: three frames per size (structured, noise, samples 0 / 1023 only), their references, the
availability set and the tables of the numpy restatement (tests/intra_ref.py), computed once."""
from functools import lru_cache

import numpy as np

import intra_ref as I
import mipgpu
import oracle_lib as O
from mipgpu.synth import synth_frame

FILTER = "filterFrame_1d_int"
TABLES = ("cost", "sad", "satd")


def extremes_frame(w, h, seed):
    """Samples 0 or 1023 only, in 4x4 patches with single-sample flips."""
    rng = np.random.default_rng(seed)
    f = np.repeat(np.repeat(rng.integers(0, 2, (h // 4, w // 4)), 4, axis=0), 4, axis=1)
    return ((f ^ (rng.random((h, w)) < 0.1)) * 1023).astype(np.uint16)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@lru_cache(maxsize=None)
def frames(w, h, n=3):
    kinds = [synth_frame(w, h, 0x1A7, 0), synth_frame(w, h, 0x1A8, 1), extremes_frame(w, h, 0x1A9)]
    return _freeze(np.stack(kinds[:n]))[0]


@lru_cache(maxsize=None)
def case(w, h, filt, n=3):
    """(frames [n, H, W], references (the oracle's filter `filt`, or the originals), the
    availability set, dict of the restatement's tables [n, nCTUs*5380, 2])."""
    f = frames(w, h, n)
    refs = f if filt is None else _freeze(np.stack([O.filter_frame(x, filt, 0) for x in f]))[0]
    un = mipgpu.unavailable_cus(w, h, filt)
    ref = [I.tables(x, r, un) for x, r in zip(f, refs)]
    tabs = {k: np.stack([t[k] for t in ref]) for k in TABLES}
    _freeze(un, *tabs.values())
    return f, refs, un, tabs
