"""CTU partition decision on the GPU (mip_partition_device / mip_partition_frames): all four
outputs equal the recursive restatement (tests/partition_ref.py) bit for bit on synthetic costs
-- random, ties, unavailable CUs with a CTU that has no partition, several frames -- outputs
not asked for are not written, and the device chain search -> partition -> predict gives the
reference partition's predicted frames with no host round trip."""
import numpy as np
import pytest

import mipgpu
import oracle_lib as O
import partition_cases as C
import partition_ref as R
import predict_ref as P
from mipgpu import MipEngine, layout

pytestmark = pytest.mark.gpu

FILTER = "filterFrame_1d_int"
FILL = 0xABCD
GUARD = 256
GUARD_BYTE = 0xA5
OUTPUTS = ("leaf", "ctu_cost", "ctu_leaves", "items")
PAD_ITEM = np.array((-1, -1, -1, 0, 0), mipgpu.PRED_ITEM)
VECTOR_PENALTY = tuple(int(v) for v in (np.arange(layout.NUM_SHAPES) * 21845) % (C.MAX_PENALTY + 1))


def _dev(a):
    import torch
    a = np.array(a, copy=True)                               # (the shared cases are read-only)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


class Arena:
    """The four outputs inside one guard-filled device buffer, so that a write outside an
    output -- or into an output that was not passed -- shows."""

    def __init__(self, nframes, nctus):
        import torch
        sizes = {"leaf": nframes * nctus * layout.CUS_PER_CTU, "ctu_cost": 4 * nframes * nctus,
                 "ctu_leaves": 4 * nframes * nctus, "items": nframes * nctus * R.MAX_LEAVES * mipgpu.PRED_ITEM.itemsize}
        self.shape = {"leaf": (nframes, -1), "ctu_cost": (nframes, nctus), "ctu_leaves": (nframes, nctus),
                      "items": (nframes, nctus, R.MAX_LEAVES)}
        self.span, at = {}, GUARD
        for key, n in sizes.items():
            self.span[key] = (at, at + n)
            at += (n + 63) // 64 * 64 + GUARD
        self.buf = torch.full((at,), GUARD_BYTE, dtype=torch.uint8, device="cuda")

    def tensor(self, key):
        a, b = self.span[key]
        return self.buf[a:b]

    def read(self, given):
        """(outputs of `given` as numpy, True if every byte outside them is still the guard)."""
        import torch
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        clean = np.ones(host.size, bool)
        out = {}
        for key in given:
            a, b = self.span[key]
            clean[a:b] = False
            dt = {"leaf": np.uint8, "items": mipgpu.PRED_ITEM}.get(key, np.int32)
            out[key] = host[a:b].view(dt).reshape(self.shape[key])
        return out, bool(np.all(host[clean] == GUARD_BYTE))


def _partition(best_cost, best_mode, w, h, penalty, given=OUTPUTS):
    arena = Arena(best_cost.shape[0], layout.num_ctus(w, h))
    mipgpu.partition_device(_dev(best_cost), w, h, penalty=penalty, best_mode=_dev(best_mode),
                            **{k: arena.tensor(k) for k in given})
    return arena.read(given)


def _same(got, ref, w, h):
    for key in OUTPUTS:
        assert np.array_equal(got[key], ref[key]), key
    pad = got["items"][np.arange(R.MAX_LEAVES)[None, None, :] >= got["ctu_leaves"][:, :, None]]
    assert pad.size and np.all(pad == PAD_ITEM)              # padding entries are exactly {-1, -1, -1, 0, 0}
    C.check_legal(got["leaf"], got["ctu_cost"], got["ctu_leaves"], w, h)


# (kind, width, height, penalty, frames, CTU without a partition)
CASES = [
    ("random", 132, 132, 0, 3, None),                        # 4x4-only corner CTU
    ("random", 140, 76, VECTOR_PENALTY, 3, None),
    ("random", 264, 136, C.MID_PENALTY, 3, None),
    ("random", 128, 128, C.MAX_PENALTY, 1, None),
    ("ties", 140, 76, None, 1, None),
    ("ties", 132, 132, C.MID_PENALTY, 1, None),
    ("area", 264, 136, C.MAX_PENALTY, 1, None),
    ("holes", 264, 136, C.MID_PENALTY, 1, 1),
    ("holes", 132, 132, 0, 3, 0),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-f%d" % (c[0], c[1], c[2], c[4]))
def test_device_equals_reference(gpu_available, case):
    kind, w, h, penalty, nf, ctu = case
    c, m = C.costs(w, h, kind, nf) if ctu is None else C.impossible(w, h, ctu, nf)
    ref = C.reference(w, h, kind, penalty, nf, ctu)
    got, clean = _partition(c, m, w, h, penalty)
    assert clean
    _same(got, ref, w, h)
    if nf > 1:                                               # different costs, different partitions per frame
        assert not np.array_equal(got["leaf"][0], got["leaf"][1])
    if ctu is not None:
        assert np.all(got["ctu_cost"][:, ctu] == layout.UNAVAILABLE) and not got["ctu_leaves"][:, ctu].any()
        assert (got["ctu_cost"] != layout.UNAVAILABLE).any()


@pytest.mark.parametrize("given", [("ctu_cost",), ("leaf",), ("ctu_leaves", "items"), ("items",)], ids="+".join)
def test_outputs_not_asked_for_are_not_written(gpu_available, given):
    w, h = 140, 76
    c, m = C.costs(w, h, "random", 3)
    ref = C.reference(w, h, "random", C.MID_PENALTY, 3)
    got, clean = _partition(c, m, w, h, C.MID_PENALTY, given)
    assert clean
    for key in given:
        assert np.array_equal(got[key], ref[key]), key


def test_bad_arguments_fail_before_any_launch(gpu_available):
    w, h = 140, 76
    c, m = C.costs(w, h, "random")
    arena = Arena(1, layout.num_ctus(w, h))
    d_c, d_m = _dev(c), _dev(m)
    outs = {k: arena.tensor(k) for k in OUTPUTS}
    one_bad = np.zeros(layout.NUM_SHAPES, np.int64)
    one_bad[46] = C.MAX_PENALTY + 1
    for pen in (C.MAX_PENALTY + 1, -1, one_bad):
        with pytest.raises(mipgpu.MipError, match="penalty"):
            mipgpu.partition_device(d_c, w, h, penalty=pen, best_mode=d_m, **outs)
    with pytest.raises(mipgpu.MipError, match="best_mode"):
        mipgpu.partition_device(d_c, w, h, items=outs["items"])
    with pytest.raises(mipgpu.MipError, match="no output"):
        mipgpu.partition_device(d_c, w, h, best_mode=d_m)
    _, clean = arena.read(())
    assert clean
    frame = C.real_frames()[0]
    with MipEngine(C.REAL_W, C.REAL_H, best_k=2) as eng:
        with pytest.raises(mipgpu.MipError, match="best_k"):
            eng.partition(frame)
    with MipEngine(C.REAL_W, C.REAL_H) as eng:
        with pytest.raises(mipgpu.MipError, match="penalty"):
            eng.partition(frame, penalty=C.MAX_PENALTY + 1)


# ---------------------------------------------------------------- search -> partition -> predict
def _device_chain(eng, frames, penalty, refs=None, batch=None):
    """Decisions-only search, partition and prediction of `frames` on the device: numpy dict of
    the decisions, the partition outputs, the canvas and the skipped counter."""
    import torch
    nf, h, w = frames.shape
    nct, ncu = eng.nctus, eng.cus_per_frame
    d_frames = _dev(frames)
    d_refs = None if refs is None else _dev(refs)
    bm = torch.full((nf, ncu), 0x5A, dtype=torch.uint8, device="cuda")
    bc = torch.full((nf, ncu), -3, dtype=torch.int32, device="cuda")
    step = batch or nf
    for f0 in range(0, nf, step):
        eng.search_device(d_frames[f0:f0 + step], refs=None if d_refs is None else d_refs[f0:f0 + step], costs=False,
                          best_mode=bm[f0:f0 + step], best_cost=bc[f0:f0 + step])
    arena = Arena(nf, nct)
    mipgpu.partition_device(bc, w, h, penalty=penalty, best_mode=bm, **{k: arena.tensor(k) for k in OUTPUTS})
    canvas = torch.full((nf * w * h + GUARD,), FILL - 65536, dtype=torch.int16, device="cuda")
    sk = torch.zeros(1, dtype=torch.int32, device="cuda")
    if batch is None:
        eng.predict_device(d_frames, arena.tensor("items"), canvas[:nf * w * h], refs=d_refs, skipped=sk)
    eng.check_input()
    out, clean = arena.read(OUTPUTS)
    assert clean
    out.update(best_mode=bm.cpu().numpy(), best_cost=bc.cpu().numpy(), canvas=canvas.cpu().numpy().view(np.uint16),
               skipped=int(sk.item()))
    return out


def _expected_canvas(frames, refs, ref, best_mode):
    """The blocks of tests/predict_ref.py placed by the reference partition's leaves."""
    nf, h, w = frames.shape
    want = np.full(nf * w * h, FILL, np.uint16).reshape(nf, h, w)
    f, k = np.nonzero(ref["leaf"])
    shape, x, y, bw, bh = layout.cu_geometry(w, h, k)
    for i in range(k.size):
        blk = P.CuPredictor(refs[f[i]], x[i], y[i], shape[i]).predict(best_mode[f[i], k[i]])
        assert np.all(want[f[i], y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] == FILL)      # leaves do not overlap
        want[f[i], y[i]:y[i] + bh[i], x[i]:x[i] + bw[i]] = blk
    return want.reshape(-1)


def _check_chain(got, frames, refs, decisions, ref, penalty):
    nf, h, w = frames.shape
    bm, bc = decisions
    assert np.array_equal(got["best_mode"], bm[:nf]) and np.array_equal(got["best_cost"], bc[:nf])
    for key in OUTPUTS:
        assert np.array_equal(got[key], ref[key][:nf]), key
    C.check_legal(got["leaf"], got["ctu_cost"], got["ctu_leaves"], w, h)
    # ctu_cost is the sum of best_cost + penalty over the CTU's leaves
    f, k = np.nonzero(got["leaf"])
    sums = np.zeros(got["ctu_cost"].shape, np.int64)
    np.add.at(sums, (f, k // layout.CUS_PER_CTU), got["best_cost"][f, k].astype(np.int64) + penalty)
    has = got["ctu_cost"] != layout.UNAVAILABLE
    assert np.array_equal(sums[has], got["ctu_cost"][has]) and not sums[~has].any()
    want = _expected_canvas(frames, refs, {"leaf": ref["leaf"][:nf]}, bm)
    assert np.array_equal(got["canvas"][:want.size], want)
    assert np.all(got["canvas"][want.size:] == FILL)
    assert got["skipped"] == got["items"].size - int(got["ctu_leaves"].sum())
    return has, want


def test_device_chain_gives_the_predicted_frames(gpu_available):
    """264x136, 2 frames, no filter: every CTU has a partition, so every sample of the frames
    is predicted."""
    frames = C.real_frames()[:2]
    with MipEngine(C.REAL_W, C.REAL_H, max_batch=2) as eng:
        got = _device_chain(eng, frames, C.REAL_PENALTY)
    has, want = _check_chain(got, frames, frames, C.real_decisions(), C.real_reference(), C.REAL_PENALTY)
    assert has.all() and not (want == FILL).any()


def test_device_chain_with_the_engine_filter(gpu_available):
    """The engine's separable filter at a height that is no multiple of 32 leaves the CUs that
    read the last frame rows unavailable: CTUs whose in-frame part cannot be tiled have no
    partition -- determined here on the CPU from mip_unavailable_cus alone -- and stay unwritten."""
    w, h = C.REAL_W, C.REAL_H
    assert h % 32
    un = mipgpu.unavailable_cus(w, h, FILTER)
    tileable = R.partition_frames(np.where(un, layout.UNAVAILABLE, 0).astype(np.int32)[None], w, h)["ctu_cost"][0]
    tileable = tileable != layout.UNAVAILABLE
    assert tileable.any() and not tileable.all()
    frames = C.real_frames()[:2]
    refs = np.stack([O.filter_frame(f, FILTER, 0) for f in frames])
    with MipEngine(w, h, filter=FILTER, max_batch=2) as eng:
        got = _device_chain(eng, frames, C.REAL_PENALTY)
    has, want = _check_chain(got, frames, refs, C.real_decisions(FILTER), C.real_reference(FILTER), C.REAL_PENALTY)
    assert np.array_equal(has, np.broadcast_to(tileable, has.shape))
    assert (want == FILL).any() and (want != FILL).any()


@pytest.mark.parametrize("source", [FILTER, "caller"])
def test_host_call_equals_the_device_chain(gpu_available, source):
    """MipEngine.partition of 3 frames on an engine with max_batch = 2 (two chunks), with the
    engine's filter and with caller-supplied references."""
    frames = C.real_frames()
    refs = frames[::-1] if source == "caller" else None
    with MipEngine(C.REAL_W, C.REAL_H, filter=None if source == "caller" else FILTER, max_batch=2) as eng:
        host = eng.partition(frames, penalty=C.REAL_PENALTY, refs=refs)
        dev = _device_chain(eng, frames, C.REAL_PENALTY, refs=refs, batch=2)
        again = eng.partition(frames[1:], penalty=C.REAL_PENALTY, refs=None if refs is None else refs[1:])
    bm, bc = C.real_decisions(source)
    ref = C.real_reference(source)
    for key, want in (("best_mode", bm), ("best_cost", bc), ("leaf", ref["leaf"]), ("ctu_cost", ref["ctu_cost"]),
                      ("ctu_leaves", ref["ctu_leaves"])):
        assert np.array_equal(host[key], want), key
        assert np.array_equal(dev[key], want), key
        assert np.array_equal(again[key], want[1:]), key
