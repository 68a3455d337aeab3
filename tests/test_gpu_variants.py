"""Every compiled instance of mip_search_kernel<ALT, DEC, PF, NW> against the C oracle, with
the launch census (MipEngine.search_census, mip_search_census) as the proof of which instance
served the call.

libmipgpu.so holds 16 instances: the 12-wave kernel ({orig, alt} x {table, decisions}, orig
also prefetching), the 16-wave kernel of small launches ({orig, alt} x {table, decisions}) and
the 8-wave four-wave twin of the host pipeline (as the 12-wave set).  Which one a call gets is
decided by its size, its API and a handful of knobs (mipgpu.cpp pick_work / wide_launch over work_plan.h,
pipe_kernel, mip_search.hip launch_search); CELLS names, per instance, one recipe of knobs
that reaches it on 264x200 frames -- 3x2 CTUs, partial CTUs on both axes, a width that is not a
multiple of 128 (wrapped reads; with alternative references the CUs that read the last two
columns go to the exact per-CU kernel) -- and every cell

  1. takes the census, runs the search, takes the census again: the difference must name
     exactly the expected instance (every other instance 0) and the expected pair-mode /
     chunked-queue / item-order flags;
  2. compares every frame bit for bit with the oracle: cost, SAD, SATD and the decisions (table
     cells), or the decisions written into sentinel-filled outputs (decisions-only cells).

The "large" cells are the production configuration (one slice, raster order, eight queue
chunks, prefetch) at 1/32 scale: MIPGPU_GROUPS=16 workgroups over 22 frames = 528 items, i.e.
33 items per workgroup (>= 32: the prefetching instances) in 8 chunks of 66 items, so both
the early prefetches and the late takes at a chunk's end occur.

Only four distinct frames exist (three of uniform noise and the 0/1023 checkerboard of
test_extreme_content_clipping); they are placed in a non-periodic order, so a launch that
reads or writes the wrong frame fails while the oracle runs once per distinct frame.

Alternative references come from the engine's filterFrame_2d_float_5x5_quarterCtu, KernelIdx
2 (whose outputs stay within 10 bits here: the last-column CUs run the exact kernel, but the
samples above 10 bits that only the separable filters produce are covered by
test_gpu_parity.py's 416x240 cases, not here), and from caller-supplied frames (check_refs),
one cell per wave count."""
import functools
import os
import re

import numpy as np
import pytest

import kernel_resources
import oracle_lib as O
from mipgpu import MipEngine, MipError, layout, pinned_empty
from mipgpu.synth import synth_frames

W, H = 264, 200
FILT, KIDX = "filterFrame_2d_float_5x5_quarterCtu", 2
LIB = os.path.join(os.path.dirname(__file__), "..", "vvc-mip-gpu_amd", "lib", "libmipgpu.so")

# frame of the launch -> distinct frame (3 = the checkerboard)
SEQ = {3: [2, 3, 0],
       22: [0, 3, 1, 2, 2, 0, 3, 1, 1, 1, 0, 2, 3, 3, 2, 0, 1, 0, 2, 3, 0, 1]}
CALLER_REFS = [3, 0, 1]  # caller-supplied references of the 3-frame cells: distinct frames again
BAD_Y, BAD_X = 40, 150   # the sample above 10 bits of the input-contract calls (CTU 1 of the last frame)

WIDE = {"MIPGPU_WIDE": "1"}
NARROW = {"MIPGPU_WIDE": "0"}
LARGE = {"MIPGPU_ORDER": "0", "MIPGPU_GROUPS": "16", "MIPGPU_QUEUE_CHUNKS": "8"}
TWIN = {"MIPGPU_PIPE_KERNEL": "8"}


def _cell(name, knobs, api, n, refs, dec, key, pair=False, chunked=False, ordered=False, contract=False):
    return dict(name=name, knobs=knobs, api=api, n=n, refs=refs, dec=dec, key=key, pair=pair, chunked=chunked,
                ordered=ordered, contract=contract)


def _group(prefix, knobs, api, n, waves, large):
    """The cells of one kernel width: {orig, engine-filtered} x {table, decisions}; large: the
    original-reference cells prefetch (and check the input contract in the decisions cell)."""
    flags = dict(chunked=True) if large else dict(ordered=True)
    out = []
    for refs, alt in (("orig", 0), ("engine", 1)):
        for dec in (0, 1):
            pf = int(large and not alt)
            out.append(_cell("%s-%s-%s" % (prefix, refs, "dec" if dec else "table"), knobs, api, n, refs, bool(dec),
                             (waves, alt, dec, pf), pair=waves == 16 and not alt, contract=bool(pf and dec), **flags))
    return out


CELLS = (
    # 16-wave kernel: every small launch (host API; pair mode with original references)
    _group("w16", WIDE, "host", 3, 16, False)
    + [_cell("w16-orig-table-nopair", {**WIDE, "MIPGPU_PAIR": "0"}, "host", 3, "orig", False, (16, 0, 0, 0), ordered=True),
       _cell("w16-orig-dec-nopair", {**WIDE, "MIPGPU_PAIR": "0"}, "host", 3, "orig", True, (16, 0, 1, 0), ordered=True),
       _cell("w16-caller-table", WIDE, "host", 3, "caller", False, (16, 1, 0, 0), ordered=True)]
    # 12-wave kernel, small-launch form: longest-first order, one queue counter (device API)
    + _group("w12s", NARROW, "device", 3, 12, False)
    + [_cell("w12s-caller-table", NARROW, "device", 3, "caller", False, (12, 1, 0, 0), ordered=True)]
    # 12-wave kernel, large-launch form in miniature: raster order, chunked queue, prefetch
    + _group("w12l", LARGE, "device", 22, 12, True)
    # the four-wave twin (8-wave workgroups; host pipeline only), both forms
    + _group("w8s", {**NARROW, **TWIN}, "host", 3, 8, False)
    + [_cell("w8s-caller-table", {**NARROW, **TWIN}, "host", 3, "caller", False, (8, 1, 0, 0), ordered=True)]
    + _group("w8l", {**LARGE, **TWIN}, "host", 22, 8, True)
)


def test_cells_cover_exactly_the_compiled_instances():
    """CPU: the census keys CELLS expects are exactly the mip_search_kernel instances in the
    library's code objects -- a new instance without a cell, or a cell whose instance is gone,
    fails here."""
    assert os.path.exists(LIB), "libmipgpu.so is not built"
    built = set()
    for name in kernel_resources.kernels(LIB):
        m = re.search(r"mip_search_kernelILb(\d)ELb(\d)ELb(\d)ELi(\d+)EE", name)  # <ALT, DEC, PF, NW>
        if m:
            built.add((int(m.group(4)), int(m.group(1)), int(m.group(2)), int(m.group(3))))
    assert len(built) == 16
    assert {c["key"] for c in CELLS} == built
    assert len({c["name"] for c in CELLS}) == len(CELLS)
    assert sum(c["contract"] for c in CELLS) == 2  # the two prefetching decisions-only instances


def test_census_rejects_bad_arguments():
    """CPU: mip_search_census checks its arguments before it touches the engine."""
    import mipgpu
    lib = mipgpu.library()
    assert lib.mip_search_census(None, None, 0) != 0
    assert b"bad arguments" in lib.mip_last_error()


@functools.lru_cache(maxsize=None)
def _distinct():
    from test_gpu_parity import _extreme  # the 0/1023 patterns of test_extreme_content_clipping
    fr = [f for f in synth_frames(W, H, 3, 0x7A21, 1)]
    fr.append(_extreme("checker1", W, H).astype(np.uint16))
    for f in fr:
        f.setflags(write=False)
    return tuple(fr)


@functools.lru_cache(maxsize=None)
def _want(refs, i, j=-1):
    """The oracle's (cost, sad, satd, best_mode, best_cost) of distinct frame i with original
    references, the engine's filter, or caller-supplied references = distinct frame j."""
    fr = _distinct()
    if refs == "engine":
        t = O.engine_search(fr[i], FILT, KIDX, want_sad_satd=True)
    else:
        t = O.search(fr[i], fr[j] if refs == "caller" else None, want_sad_satd=True)
    bm, bc = layout.best_modes(t[0], layout.num_ctus(W, H))
    for a in (*t, bm, bc):
        a.setflags(write=False)
    return (*t, bm, bc)


def _delta(before, after):
    return {k: after[k] - before[k] for k in after}


def _assert_census(d, c, launches_at_least=1):
    ran = {k: v for k, v in d.items() if isinstance(k, tuple) and v}
    assert set(ran) == {c["key"]}, (c["name"], ran)
    n = ran[c["key"]]
    assert n >= launches_at_least, (c["name"], ran)
    for flag in ("pair", "chunked", "ordered"):
        assert d[flag] == (n if c[flag] else 0), (c["name"], flag, d[flag], n)


def _assert_outputs(c, out):
    """out: numpy arrays per key, [frames, ...]."""
    seq = SEQ[c["n"]]
    for f, i in enumerate(seq):
        cost, sad, satd, bm, bc = _want(c["refs"], i, CALLER_REFS[f] if c["refs"] == "caller" else -1)
        if not c["dec"]:
            assert np.array_equal(out["cost"][f], cost), (c["name"], f, "cost")
            assert np.array_equal(out["sad"][f], sad), (c["name"], f, "sad")
            assert np.array_equal(out["satd"][f], satd), (c["name"], f, "satd")
        assert np.array_equal(out["best_mode"][f], bm), (c["name"], f, "best_mode")
        assert np.array_equal(out["best_cost"][f], bc), (c["name"], f, "best_cost")


def _host_buffers(eng, c, frames, refs):
    """Inputs and sentinel-filled outputs of a host-API call.  The 22-frame calls use
    page-locked buffers: a whole slot's frames then go as one chunk (pageable transfers are
    cut to the bounce ring's size)."""
    n = c["n"]
    pinned = n > 3
    empty = pinned_empty if pinned else (lambda shape, dt: np.empty(shape, dt))
    if pinned:
        pf = pinned_empty(frames.shape, np.uint16)
        pf[:] = frames
        frames = pf
    out = {"best_mode": empty((n, eng.cus_per_frame), np.uint8), "best_cost": empty((n, eng.cus_per_frame), np.int32)}
    if not c["dec"]:
        for key in ("cost", "sad", "satd"):
            out[key] = empty((n, eng.costs_per_frame), np.int32)
    return frames, refs, out


def _sentinel(out):
    for key, a in out.items():
        a[...] = 0x5a if key == "best_mode" else -5


def _run_host(eng, c, frames, refs, out):
    _sentinel(out)
    return eng.search(frames, refs=refs, costs=not c["dec"], best=True, sad_satd=not c["dec"], out=out)


def _run_device(eng, c, d_frames, d_refs):
    import torch
    n = c["n"]
    out = {"best_mode": torch.full((n, eng.cus_per_frame), 0x5a, dtype=torch.uint8, device="cuda"),
           "best_cost": torch.full((n, eng.cus_per_frame), -5, dtype=torch.int32, device="cuda")}
    if c["dec"]:
        assert eng.search_device(d_frames, refs=d_refs, costs=False, **out) is None
    else:
        for key in ("cost", "sad", "satd"):
            out[key] = torch.full((n, eng.costs_per_frame), -5, dtype=torch.int32, device="cuda")
        eng.search_device(d_frames, refs=d_refs, costs=out["cost"], sad=out["sad"], satd=out["satd"],
                          best_mode=out["best_mode"], best_cost=out["best_cost"])
    eng.check_input()  # (waits for the stream)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("c", CELLS, ids=[c["name"] for c in CELLS])
def test_variant_vs_oracle(gpu_available, monkeypatch, c):
    for k, v in c["knobs"].items():  # (read per launch)
        monkeypatch.setenv(k, v)
    n = c["n"]
    distinct = _distinct()
    frames = np.stack([distinct[i] for i in SEQ[n]])
    refs = np.stack([distinct[j] for j in CALLER_REFS]) if c["refs"] == "caller" else None
    # host API, 22 frames: four slots of 22 frames, so the call is one unramped chunk
    max_batch = 88 if c["api"] == "host" and n == 22 else n
    filt, kidx = (FILT, KIDX) if c["refs"] == "engine" else (None, 0)
    with MipEngine(W, H, max_batch=max_batch, filter=filt, kernel_idx=kidx, want_sad_satd=not c["dec"]) as eng:
        if c["api"] == "host":
            frames_in, refs_in, out = _host_buffers(eng, c, frames, refs)
            run = lambda fr: _run_host(eng, c, fr, refs_in, out)  # noqa: E731
        else:
            import torch
            frames_in = torch.from_numpy(frames.astype(np.int16)).cuda()
            refs_in = None if refs is None else torch.from_numpy(refs.astype(np.int16)).cuda()
            run = lambda fr: _run_device(eng, c, fr, refs_in)  # noqa: E731
        c0 = eng.search_census()
        got = run(frames_in)
        c1 = eng.search_census()
        print("census %s: %s" % (c["name"], {k: v for k, v in _delta(c0, c1).items() if v}))
        _assert_census(_delta(c0, c1), c)
        _assert_outputs(c, got)
        if c["contract"]:
            # a sample above 10 bits in a prefetched window of the last frame: that call, and
            # only it, fails loudly; the engine then serves a clean call as before
            if c["api"] == "host":
                frames_in[n - 1, BAD_Y, BAD_X] = 1024
                with pytest.raises(MipError, match="above 10 bits"):
                    run(frames_in)
                frames_in[n - 1, BAD_Y, BAD_X] = frames[n - 1, BAD_Y, BAD_X]
            else:
                bad = frames_in.clone()
                bad[n - 1, BAD_Y, BAD_X] = 1024
                with pytest.raises(MipError, match="above 10 bits"):
                    run(bad)
            _assert_outputs(c, run(frames_in))
            _assert_census(_delta(c0, eng.search_census()), c, launches_at_least=3)
