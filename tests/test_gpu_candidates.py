"""K-best candidate lists on the GPU (mip_candidates_device / mip_candidates_frames): both outputs
equal the numpy restatement (tests/candidates_ref.py, pinned by tests/test_candidates_cpu.py) bit
for bit on synthetic tables full of ties for every subset of the families, k in {1, 2, 3, 8, 32}
and kin in {1, 3, 32}, with one output only, at the top of the value domain, and on a launch whose
CU count leaves the last workgroup short; on the real tables of the search, intra_device,
angular_device and angular_refine_device they equal the restatement computed from the C oracle,
tests/intra_ref.py and tests/angular_ref.py / tests/angular_refine_ref.py, and with k = 1 the
decisions the existing merges leave; the host call equals the device path across a chunk
boundary; bad arguments are refused before any launch.  Outputs live in guard-filled arenas."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

import angular_cases as AC
import angular_refine_cases as RC
import candidates_ref as C
import intra_cases as IC
import mipgpu
import oracle_lib as O
from mipgpu import MipEngine, layout

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements before and after every output
GUARD_WORD, GUARD_BYTE = -0x5A5A5A5B, 0x5A
UN = layout.UNAVAILABLE
FAMILIES = (("mip_mode", "mip_cost"), ("intra_cost",), ("ang_cost",))
W, H, NF = 136, 72, 3
INTRA_BIAS, ANG_BIAS = (3, 5), 9


def _dev(a):
    import torch
    a = np.array(a, copy=True)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


class Arena:
    """modes inside a guard-filled uint8 device buffer, costs inside a guard-filled int32 one."""

    def __init__(self, nframes, ncu, k):
        import torch
        self.shape = (nframes, ncu, k)
        n = nframes * ncu * k
        self.bytes = torch.full((n + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.words = torch.full((n + 2 * GUARD,), GUARD_WORD, dtype=torch.int32, device="cuda")
        self.modes, self.costs = self.bytes[GUARD:GUARD + n], self.words[GUARD:GUARD + n]

    def read(self, modes=True, costs=True):
        """(modes, costs, True if everything outside the outputs that were given is still the guard)."""
        import torch
        torch.cuda.synchronize()
        b, w = self.bytes.cpu().numpy(), self.words.cpu().numpy()
        inner_b, inner_w = b[GUARD:-GUARD], w[GUARD:-GUARD]
        clean = bool(np.all(b[:GUARD] == GUARD_BYTE) and np.all(b[-GUARD:] == GUARD_BYTE) and np.all(w[:GUARD] == GUARD_WORD) and
                     np.all(w[-GUARD:] == GUARD_WORD) and (modes or np.all(inner_b == GUARD_BYTE)) and (costs or np.all(inner_w == GUARD_WORD)))
        return inner_b.reshape(self.shape), inner_w.reshape(self.shape), clean


def _subset(tables, s):
    return {key: tables[key] for f in range(3) if s >> f & 1 for key in FAMILIES[f]}


def _call(w, h, k, part, arena, intra_bias=None, ang_bias=0, modes=True, costs=True):
    mipgpu.candidates_device(w, h, k, intra_bias=intra_bias, ang_bias=ang_bias, modes=arena.modes if modes else False,
                             costs=arena.costs if costs else False, **part)
    return arena.read(modes, costs)


# ---------------------------------------------------------------- 1. synthetic tables
@pytest.mark.parametrize("kin", (1, 3, 32))
@pytest.mark.parametrize("geometry", ((136, 72), (60, 36)), ids=lambda g: "%dx%d" % g)
def test_synthetic_tables_equal_the_restatement(gpu_available, geometry, kin):
    w, h = geometry
    ncu = layout.num_ctus(w, h) * layout.CUS_PER_CTU
    host = C.synthetic(NF * ncu, kin, 7 * kin + w)
    host = {key: v.reshape(NF, ncu, -1) for key, v in host.items()}
    # what the test is about is really in its inputs
    n = C.count(**host)
    m3, c3 = C.candidates(3, **host)
    fam_of = np.where(m3 < 32, 0, np.where(m3 >= 0xF0, 1, 2))
    assert (n == 0).any() and ((n > 0) & (n < 3)).any() and (n > 32).any()
    assert ((c3[..., 0] == c3[..., 1]) & (c3[..., 0] != UN) & (fam_of[..., 0] != fam_of[..., 1])).mean() > 0.2
    assert ((host["mip_mode"] > 31) & (host["mip_mode"] != 0xFF)).any() and (host["mip_mode"] == 0xFF).any()
    dev = {key: _dev(v) for key, v in host.items()}
    for s in range(1, 8):
        part, hpart = _subset(dev, s), _subset(host, s)
        for k in (1, 2, 3, 8, 32):
            bias, ab = (((1, 0), 2) if k == 3 else (None, 0))
            want = C.candidates(k, intra_bias=bias if "intra_cost" in hpart else None, ang_bias=ab, **hpart)
            got_m, got_c, clean = _call(w, h, k, part, Arena(NF, ncu, k), bias, ab)
            assert clean, (s, k)
            assert np.array_equal(got_m, want[0]) and np.array_equal(got_c, want[1]), (s, k)
    want = C.candidates(3, **host)                            # one output only
    got_m, got_c, clean = _call(w, h, 3, dev, Arena(NF, ncu, 3), costs=False)
    assert clean and np.array_equal(got_m, want[0])
    got_m, got_c, clean = _call(w, h, 3, dev, Arena(NF, ncu, 3), modes=False)
    assert clean and np.array_equal(got_c, want[1])


# ---------------------------------------------------------------- 2. top of the domain
def test_top_of_the_domain(gpu_available):
    w, h = 136, 72
    ncu = layout.num_ctus(w, h) * layout.CUS_PER_CTU
    host = {key: v.reshape(NF, ncu, -1) for key, v in C.top_of_domain(NF * ncu, 3).items()}
    bias, ab = (C.MAX_BIAS, C.MAX_BIAS), C.MAX_BIAS
    want = C.candidates(32, intra_bias=bias, ang_bias=ab, **host)
    assert want[1][want[1] != UN].max() == (1 << 24) - 1 and (want[1] == 0).any() and (want[1] == 8380416 + C.MAX_BIAS).any()
    got_m, got_c, clean = _call(w, h, 32, {key: _dev(v) for key, v in host.items()}, Arena(NF, ncu, 32), bias, ab)
    assert clean and np.array_equal(got_m, want[0]) and np.array_equal(got_c, want[1])


# ---------------------------------------------------------------- 3. beyond one workgroup row
def test_many_workgroups_and_a_short_last_one(gpu_available):
    """The launcher takes one 64-lane workgroup per 64 CUs (tests/test_candidates_cpu.py pins that
    to its text): 7 frames of 60x36 are 37 660 CUs, 588 whole workgroups and one of 28 lanes, the
    other 36 of which must neither read nor write.  Frames repeat from a pool of three."""
    w, h, kin, k = 60, 36, 3, 3
    ncu = layout.num_ctus(w, h) * layout.CUS_PER_CTU
    pool = {key: v.reshape(3, ncu, -1) for key, v in C.synthetic(3 * ncu, kin, 41).items()}
    want = C.candidates(k, intra_bias=INTRA_BIAS, ang_bias=ANG_BIAS, **pool)
    sel = np.array([0, 1, 2, 2, 0, 1, 1])
    assert (sel.size * ncu) % 64 == 28 and sel.size * ncu // 64 == 588
    arena = Arena(sel.size, ncu, k)
    got_m, got_c, clean = _call(w, h, k, {key: _dev(v[sel]) for key, v in pool.items()}, arena, INTRA_BIAS, ANG_BIAS)
    assert clean and np.array_equal(got_m, want[0][sel]) and np.array_equal(got_c, want[1][sel])


# ---------------------------------------------------------------- 4. real tables
@lru_cache(maxsize=None)
def real_reference(filt):
    """The families' tables at 136x72 from the existing references: the C oracle's costs as lists of
    three (layout.topk_modes), tests/intra_ref.py, tests/angular_ref.py with all 65 modes and
    tests/angular_refine_ref.py (even list, two seeds)."""
    frames, _, un, ang = AC.case(W, H, filt)
    intra = IC.case(W, H, filt)[3]["cost"]
    nct = layout.num_ctus(W, H)
    lists = [layout.topk_modes(O.engine_search(f, filt), nct, 3) for f in frames]
    ref = {"frames": frames, "un": un, "mip_mode": np.stack([m for m, _ in lists]), "mip_cost": np.stack([c for _, c in lists]),
           "intra_cost": intra, "ang_cost": ang["cost"], "fine_cost": RC.refined(W, H, filt, "even", 2)["cost"]}
    for k in (1, 3):
        for name in ("ang_cost", "fine_cost"):
            ref[name, k] = C.candidates(k, ref["mip_mode"][..., :k], ref["mip_cost"][..., :k], intra, INTRA_BIAS, ref[name], ANG_BIAS)
    return ref


@pytest.mark.parametrize("filt", (None, IC.FILTER), ids=("orig", "1d_int"))
def test_real_tables(gpu_available, filt):
    import torch
    ref = real_reference(filt)
    ncu = ref["un"].size
    with MipEngine(W, H, filter=filt, max_batch=NF, best_k=3) as eng:
        d_frames = _dev(ref["frames"])
        mip_mode = torch.empty((NF, ncu, 3), dtype=torch.uint8, device="cuda")
        mip_cost = torch.empty((NF, ncu, 3), dtype=torch.int32, device="cuda")
        table = eng.search_device(d_frames, best_mode=mip_mode, best_cost=mip_cost)
        intra = torch.empty((NF, ncu, 2), dtype=torch.int32, device="cuda")
        eng.intra_device(d_frames, cost=intra)
        ang = torch.empty((NF, ncu, 65), dtype=torch.int32, device="cuda")
        eng.angular_device(d_frames, cost=ang)
        fine = torch.empty((NF, ncu, 65), dtype=torch.int32, device="cuda")
        eng.angular_refine_device(d_frames, modes=mipgpu.ANGULAR_EVEN_MODES, seeds=2, cost=fine)
        assert np.array_equal(mip_mode.cpu().numpy(), ref["mip_mode"]) and np.array_equal(fine.cpu().numpy(), ref["fine_cost"])
        best_mode, best_cost = mipgpu.topk_device(table, W, H, 1)       # the K = 1 decisions of the same search
        for name, d_ang in (("ang_cost", ang), ("fine_cost", fine)):
            arena = Arena(NF, ncu, 3)
            mipgpu.candidates_device(W, H, 3, mip_mode, mip_cost, intra, INTRA_BIAS, d_ang, ANG_BIAS, arena.modes, arena.costs)
            got_m, got_c, clean = arena.read()
            want = ref[name, 3]
            assert clean and np.array_equal(got_m, want[0]) and np.array_equal(got_c, want[1]), name
            assert (got_m[..., 0] < 32).any() and (got_m[..., 0] >= 0xF0).any() and ((got_m[..., 0] >= 0x82) & (got_m[..., 0] <= 0xC2)).any()
            assert np.all(got_m[:, ref["un"]] == 0xFF) and np.all(got_c[:, ref["un"]] == UN) and np.all(got_m[:, ~ref["un"]] != 0xFF)
            # k = 1, kin = 1 against the existing chain: search -> intra merge -> angular merge
            bm, bc = best_mode.clone().reshape(NF, ncu), best_cost.clone().reshape(NF, ncu)
            eng.intra_device(d_frames, bias=INTRA_BIAS, best_mode=bm, best_cost=bc)
            if name == "ang_cost":
                eng.angular_device(d_frames, bias=ANG_BIAS, best_mode=bm, best_cost=bc)
            else:
                eng.angular_refine_device(d_frames, modes=mipgpu.ANGULAR_EVEN_MODES, seeds=2, bias=ANG_BIAS, best_mode=bm, best_cost=bc)
            arena = Arena(NF, ncu, 1)
            mipgpu.candidates_device(W, H, 1, mip_mode[..., :1].contiguous(), mip_cost[..., :1].contiguous(), intra, INTRA_BIAS, d_ang,
                                     ANG_BIAS, arena.modes, arena.costs)
            got_m, got_c, clean = arena.read()
            assert clean and np.array_equal(got_m[..., 0], bm.cpu().numpy()) and np.array_equal(got_c[..., 0], bc.cpu().numpy()), name
            assert np.array_equal(got_m, ref[name, 1][0]) and np.array_equal(got_c, ref[name, 1][1]), name
        eng.check_input()


# ---------------------------------------------------------------- 5. host call
def test_host_call_equals_the_device_path(gpu_available):
    ref = real_reference(None)
    frames = ref["frames"]
    flat = ref["mip_mode"], ref["mip_cost"]
    for max_batch in (3, 2):                                  # 2: chunks of 2 + 1 frames
        with MipEngine(W, H, max_batch=max_batch) as eng:
            plain = eng.candidates(frames, k=3, angular="all", intra_bias=INTRA_BIAS, angular_bias=ANG_BIAS)
            fine = eng.candidates(frames, k=3, angular=mipgpu.ANGULAR_EVEN_MODES, seeds=2, intra_bias=INTRA_BIAS, angular_bias=ANG_BIAS)
            caller = eng.candidates(frames, k=3, angular="all", intra_bias=INTRA_BIAS, angular_bias=ANG_BIAS, refs=frames)
            one = eng.candidates(frames, k=1, angular="all", intra_bias=INTRA_BIAS, angular_bias=ANG_BIAS)   # decisions-only search
            seed1 = eng.candidates(frames, k=3, angular=mipgpu.ANGULAR_EVEN_MODES, seeds=1)
            regular = eng.candidates(frames, k=3)
            alone = eng.candidates(frames, k=3, regular=False)                                               # flags == 0
        for got, want in ((plain, ref["ang_cost", 3]), (fine, ref["fine_cost", 3]), (caller, ref["ang_cost", 3]), (one, ref["ang_cost", 1]),
                          (seed1, C.candidates(3, *flat, ref["intra_cost"], None, RC.refined(W, H, None, "even", 1)["cost"], 0)),
                          (regular, C.candidates(3, *flat, ref["intra_cost"])), (alone, flat)):
            assert sorted(got) == ["costs", "modes"]
            assert np.array_equal(got["modes"], want[0]) and np.array_equal(got["costs"], want[1]), max_batch
    with MipEngine(W, H, max_batch=2, best_k=3) as eng:       # flags == 0: the search's own best_k lists
        own = eng.search(frames, costs=False, best=True)
        alone = eng.candidates(frames, k=3, regular=False)
        one = eng.candidates(frames, k=1, angular="all", intra_bias=INTRA_BIAS, angular_bias=ANG_BIAS)       # a table, lists of one
    assert np.array_equal(alone["modes"], own["best_mode"].reshape(alone["modes"].shape))
    assert np.array_equal(alone["costs"], own["best_cost"].reshape(alone["costs"].shape))
    assert np.array_equal(one["modes"], ref["ang_cost", 1][0]) and np.array_equal(one["costs"], ref["ang_cost", 1][1])
    with MipEngine(W, H, filter=IC.FILTER, max_batch=2) as eng:
        ref = real_reference(IC.FILTER)
        fine = eng.candidates(frames, k=3, angular=mipgpu.ANGULAR_EVEN_MODES, seeds=2, intra_bias=INTRA_BIAS, angular_bias=ANG_BIAS)
    assert np.array_equal(fine["modes"], ref["fine_cost", 3][0]) and np.array_equal(fine["costs"], ref["fine_cost", 3][1])


# ---------------------------------------------------------------- 6. argument rules
def test_argument_rules(gpu_available):
    """Every bad call is refused before any launch and writes nothing."""
    import torch
    w, h, kin, k = 60, 36, 3, 3
    ncu = layout.num_ctus(w, h) * layout.CUS_PER_CTU
    t = {key: _dev(v.reshape(1, ncu, -1)) for key, v in C.synthetic(ncu, kin, 1).items()}
    arena = Arena(1, ncu, 32)                                 # (room for any k of the calls below)
    L = mipgpu.library()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = {key: v.data_ptr() for key, v in t.items()}
    bias = (ctypes.c_int32 * 2)
    good = dict(k=k, mip_mode=p["mip_mode"], mip_cost=p["mip_cost"], kin=kin, intra=p["intra_cost"], intra_bias=None, ang=p["ang_cost"],
                ang_bias=0, modes=arena.modes.data_ptr(), costs=arena.costs.data_ptr())

    def call(**change):
        a = dict(good, **change)
        rc = L.mip_candidates_device(w, h, 1, a["k"], a["mip_mode"], a["mip_cost"], a["kin"], a["intra"], a["intra_bias"], a["ang"],
                                     a["ang_bias"], a["modes"], a["costs"], s)
        return rc, L.mip_last_error().decode()

    for change, text in ((dict(k=0), "k must"), (dict(k=33), "k must"), (dict(kin=0), "kin must"), (dict(kin=33), "kin must"),
                         (dict(mip_mode=None), "together"), (dict(mip_cost=None), "together"),
                         (dict(mip_mode=None, mip_cost=None, intra=None, ang=None), "no family"), (dict(modes=None, costs=None), "no output"),
                         (dict(intra_bias=bias(0, -1)), "intra bias"), (dict(intra_bias=bias((1 << 20) + 1, 0)), "intra bias"),
                         (dict(ang_bias=-1), "angular bias"), (dict(ang_bias=(1 << 20) + 1), "angular bias"),
                         (dict(costs=arena.costs.data_ptr() + 2), "aligned"), (dict(modes=p["mip_mode"]), "overlaps"),
                         (dict(costs=p["ang_cost"] + 4 * (ncu * 65 - 1)), "overlaps")):
        rc, err = call(**change)
        assert rc != 0 and text in err, (change, err)
    assert arena.read(False, False)[2]                        # nothing was written, inside or outside the outputs
    assert call()[0] == 0 and call(intra_bias=bias(1 << 20, 0), ang_bias=1 << 20, k=32, costs=None)[0] == 0
    torch.cuda.synchronize()
    with pytest.raises(mipgpu.MipError, match="k must"):
        mipgpu.candidates_device(w, h, 33, **t)
    with pytest.raises(mipgpu.MipError, match="no family"):
        mipgpu.candidates_device(w, h, 3)
    with pytest.raises(mipgpu.MipError, match="together"):
        mipgpu.candidates_device(w, h, 3, mip_mode=t["mip_mode"])
    frames = IC.frames(w, h)
    with MipEngine(w, h, max_batch=3) as eng:
        modes, costs = np.full((3, ncu, 3), 0x5A, np.uint8), np.full((3, ncu, 3), -7, np.int32)
        even = np.array(mipgpu.ANGULAR_EVEN_MODES, np.uint8)

        def frames_call(k=3, flags=3, intra_bias=None, ang_modes=even, n=33, seeds=0, ang_bias=0, out=True):
            rc = L.mip_candidates_frames(eng._h, frames.ctypes.data, None, 3, k, flags, intra_bias, ang_modes.ctypes.data, n, seeds, ang_bias,
                                         modes.ctypes.data if out else None, costs.ctypes.data if out else None)
            return rc, L.mip_last_error().decode()

        same = np.array([20, 20], np.uint8)
        for change, text in ((dict(flags=4), "flags"), (dict(flags=0x13), "flags"), (dict(k=0), "k must"), (dict(k=33), "k must"),
                             (dict(intra_bias=bias(-1, 0)), "intra bias"), (dict(ang_bias=(1 << 20) + 1), "angular bias"),
                             (dict(ang_modes=same, n=2), "modes"), (dict(n=0), "modes"), (dict(seeds=4), "seeds"), (dict(seeds=-1), "seeds"),
                             (dict(out=False), "no output")):
            rc, err = frames_call(**change)
            assert rc != 0 and text in err, (change, err)
        assert np.all(modes == 0x5A) and np.all(costs == -7)
        # without their bit the angular arguments and the intra bias are not looked at
        assert frames_call(flags=1, ang_modes=same, n=2, seeds=9, ang_bias=-1)[0] == 0
        modes[:], costs[:] = 0x5A, -7
        assert frames_call(flags=0, intra_bias=bias(-1, -1), ang_modes=same, n=2, seeds=9, ang_bias=-1)[0] == 0
        assert not np.all(costs == -7)
        with pytest.raises(mipgpu.MipError, match="seeds"):
            eng.candidates(frames, angular="all", seeds=4)
        with pytest.raises(mipgpu.MipError, match="k must"):
            eng.candidates(frames, k=0)
