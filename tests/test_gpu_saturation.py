"""Saturating content through every compiled search-kernel instance, bit for bit against the
oracle.

Phase A of the search kernel clips the reduced predictions to [0, 1023] while it converts them
(mip_search.hip convert_pair); nothing downstream clips again.  The frames here make both
clips fire in bulk: random 0 / 1023 blocks at 4x4 granularity, 8-pixel stripes in either
direction, all 0 and all 1023, at 264x200 -- the size at which test_gpu_variants.py reaches all
16 instances -- through that file's instance recipes (original references and the engine's
filterFrame_2d_float_5x5_quarterCtu), with the launch census as the proof of the instance.

test_clips_are_exercised (CPU) restates the unclipped reduced prediction from the mip_tables.h
weights and asserts, per size id and orientation, the share of these frames' reduced samples
that lie above 1023 and below 0: at least 1 % each (they reach 15 / 16 % for sizeId 0, 13 / 13 %
for sizeId 1 and 10 / 7 % for sizeId 2, in either orientation)."""
import functools
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_variants as V
from mipgpu import MipEngine, layout

W, H = V.W, V.H
NAMES = ("blocks", "vstripes", "hstripes", "zeros", "full")
# frame of the launch -> distinct frame; the 3-frame recipes run twice to see all five
SEQ3 = ([0, 1, 2], [3, 4, 0])
SEQ22 = [0, 3, 1, 2, 4, 0, 3, 1, 1, 4, 0, 2, 3, 3, 2, 0, 1, 4, 2, 3, 0, 1]
# the four {orig, engine-filtered} x {table, decisions} recipes of each of the five groups
CELLS = [c for c in V.CELLS if c["refs"] in ("orig", "engine") and "nopair" not in c["name"]]
MIN_SHARE = 0.01


@functools.lru_cache(maxsize=None)
def _frames():
    rng = np.random.default_rng(0x5A7)
    yy, xx = np.mgrid[0:H, 0:W]
    blocks = np.kron(rng.integers(0, 2, size=(H // 4, W // 4)), np.ones((4, 4), np.int64)) * 1023
    fr = [blocks, ((xx // 8) & 1) * 1023, ((yy // 8) & 1) * 1023, np.zeros((H, W), np.int64), np.full((H, W), 1023)]
    fr = tuple(np.ascontiguousarray(f, np.uint16) for f in fr)
    for f in fr:
        f.setflags(write=False)
    return fr


# ---- the unclipped reduced prediction, restated (intra.cl:415-482 as oracle/mip_oracle.c reads it)
def _weights(name, modes, nout, nin):
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "vvc-mip-gpu_amd", "csrc", "mip_tables.h")).read()
    body = hdr[hdr.index("#define " + name):]
    vals = [int(v, 16) for v in re.findall(r"0x([0-9a-f]+)", body[body.index("{") + 1:body.index("}")])]
    return np.array(vals, np.int64).reshape(modes, nout, nin)


@functools.lru_cache(maxsize=None)
def _matrices():
    w2 = _weights("MIP_WEIGHTS_S2", 6, 64, 7)
    w2 = np.concatenate([np.zeros((6, 64, 1), np.int64), w2], axis=2)  # input 0 has no column (p_0 = 0)
    return {0: _weights("MIP_WEIGHTS_S0", 16, 16, 4), 1: _weights("MIP_WEIGHTS_S1", 8, 16, 8), 2: w2}


def _reduced_boundaries(refs, s, xs, ys):
    """redT, redL [N, rbs] of the CUs of shape s at frame positions (xs, ys), all inside the frame."""
    r = refs.astype(np.int64)
    top = np.where((ys > 0)[:, None], r[np.maximum(ys - 1, 0)[:, None], xs[:, None] + np.arange(s.w)[None, :]],
                   np.where(xs == 0, 512, r[0, np.maximum(xs - 1, 0)])[:, None])
    left = np.where((xs > 0)[:, None], r[ys[:, None] + np.arange(s.h)[None, :], np.maximum(xs - 1, 0)[:, None]],
                    np.where(ys == 0, 512, r[np.maximum(ys - 1, 0), 0])[:, None])
    rbs = 2 if s.size_id == 0 else 4
    out = []
    for src, n in ((top, s.w), (left, s.h)):
        df = n // rbs
        out.append((src.reshape(-1, rbs, df).sum(axis=2) + (df // 2 if df > 1 else 0)) >> (df.bit_length() - 1))
    return out


def _unclipped(refs):
    """{(size_id, transposed): every unclipped reduced sample ((acc >> 6) + b0) of the frame's CUs
    that lie inside the frame}."""
    cols, rows = layout.ctu_grid(W, H)
    ctu = np.arange(cols * rows)
    res = {}
    for s in layout.SHAPES:
        px, py = s.positions()
        xs = (128 * (ctu % cols)[:, None] + px[None, :]).reshape(-1)
        ys = (128 * (ctu // cols)[:, None] + py[None, :]).reshape(-1)
        keep = (xs + s.w <= W) & (ys + s.h <= H)
        red_t, red_l = _reduced_boundaries(refs, s, xs[keep], ys[keep])
        wm = _matrices()[s.size_id]
        for tr in (0, 1):
            b = np.concatenate([red_l, red_t] if tr else [red_t, red_l], axis=1)
            b0 = b[:, 0]
            p = b - b0[:, None]
            p[:, 0] = 0 if s.size_id == 2 else 512 - b0
            acc = (32 - 32 * p.sum(axis=1))[:, None, None] + np.einsum("nk,mjk->nmj", p, wm)
            res.setdefault((s.size_id, tr), []).append(((acc >> 6) + b0[:, None, None]).reshape(-1))
    return {k: np.concatenate(v) for k, v in res.items()}


def test_restatement_is_the_oracle_reduced_prediction():
    """The restatement against oracle/mip_oracle.c's mipo_reduced_pred on random boundaries: equal
    after the clip (and as a multiset per mode: the oracle stores transposed modes transposed)."""
    import predict_ref
    L = predict_ref._lib()     # (the oracle with mipo_reduced_pred's argument types set: the same call whichever test ran first)
    rng = np.random.default_rng(11)
    for sid, (modes, r, rbs) in {0: (16, 4, 2), 1: (8, 4, 4), 2: (6, 8, 4)}.items():
        wm = _matrices()[sid]
        for _ in range(20):
            rt, rl = rng.integers(0, 1024, rbs).astype(np.int16), rng.integers(0, 1024, rbs).astype(np.int16)
            for tr in (0, 1):
                b = np.concatenate([rl, rt] if tr else [rt, rl]).astype(np.int64)
                p = b - b[0]
                p[0] = 0 if sid == 2 else 512 - b[0]
                mine = np.clip(((32 - 32 * p.sum() + wm @ p) >> 6) + b[0], 0, 1023)  # [modes, r * r]
                for m in range(modes):
                    pred = np.zeros(r * r, np.int16)
                    L.mipo_reduced_pred(sid, m, tr, rt, rl, pred)
                    want = pred.reshape(r, r).T.reshape(-1) if tr else pred
                    assert np.array_equal(mine[m], want), (sid, m, tr)


def test_clips_are_exercised():
    """CPU, before any launch: per size id and orientation, at least 1 % of the reduced samples of
    the five frames lie above 1023 and at least 1 % below 0 (original references)."""
    per = [_unclipped(f) for f in _frames()]
    for key in sorted(per[0]):
        v = np.concatenate([u[key] for u in per])
        above, below = float((v > 1023).mean()), float((v < 0).mean())
        print("sizeId %d %s: %d samples, %.2f %% above 1023, %.2f %% below 0 (max %d, min %d)" %
              (key[0], "transposed" if key[1] else "plain", v.size, 100 * above, 100 * below, v.max(), v.min()))
        assert above >= MIN_SHARE and below >= MIN_SHARE, key


@functools.lru_cache(maxsize=None)
def _want(refs, i):
    fr = _frames()[i]
    if refs == "engine":
        t = O.engine_search(fr, V.FILT, V.KIDX, want_sad_satd=True)
    else:
        t = O.search(fr, None, want_sad_satd=True)
    bm, bc = layout.best_modes(t[0], layout.num_ctus(W, H))
    for a in (*t, bm, bc):
        a.setflags(write=False)
    return (*t, bm, bc)


def _assert_outputs(c, seq, out):
    for f, i in enumerate(seq):
        cost, sad, satd, bm, bc = _want(c["refs"], i)
        if not c["dec"]:
            assert np.array_equal(out["cost"][f], cost), (c["name"], NAMES[i], "cost")
            assert np.array_equal(out["sad"][f], sad), (c["name"], NAMES[i], "sad")
            assert np.array_equal(out["satd"][f], satd), (c["name"], NAMES[i], "satd")
        assert np.array_equal(out["best_mode"][f], bm), (c["name"], NAMES[i], "best_mode")
        assert np.array_equal(out["best_cost"][f], bc), (c["name"], NAMES[i], "best_cost")


@pytest.mark.gpu
@pytest.mark.parametrize("c", CELLS, ids=[c["name"] for c in CELLS])
def test_saturating_frames_vs_oracle(gpu_available, monkeypatch, c):
    for k, v in c["knobs"].items():  # (read per launch)
        monkeypatch.setenv(k, v)
    n = c["n"]
    max_batch = 88 if c["api"] == "host" and n == 22 else n  # (as test_gpu_variants: one unramped chunk)
    filt, kidx = (V.FILT, V.KIDX) if c["refs"] == "engine" else (None, 0)
    with MipEngine(W, H, max_batch=max_batch, filter=filt, kernel_idx=kidx, want_sad_satd=not c["dec"]) as eng:
        for seq in (SEQ3 if n == 3 else (SEQ22,)):
            frames = np.stack([_frames()[i] for i in seq])
            c0 = eng.search_census()
            if c["api"] == "host":
                frames_in, _, out = V._host_buffers(eng, c, frames, None)
                got = V._run_host(eng, c, frames_in, None, out)
            else:
                import torch
                got = V._run_device(eng, c, torch.from_numpy(frames.astype(np.int16)).cuda(), None)
            V._assert_census(V._delta(c0, eng.search_census()), c)
            _assert_outputs(c, seq, got)


def test_cells_cover_the_compiled_instances():
    """20 recipes (five groups of four), all 16 instances (the small and the large 12- and 8-wave
    groups share their alternative-reference instances)."""
    assert len(CELLS) == 20 and {c["key"] for c in CELLS} == {c["key"] for c in V.CELLS}
    assert len({c["key"] for c in CELLS}) == 16
