"""Planar / DC block output on the CPU (no GPU): intra_predict_cu_host of csrc/intra_plan.h -- the
steps of the prediction kernel's regular items, from the per-sample functions the kernel itself
calls -- compiled stand-alone (tests/cpp/test_intra_predict.cpp, with
-fsanitize=address,undefined; no preloaded library).  Every available CU of all 47 shapes, both
modes, equals tests/intra_ref.predict bit for bit, and the SAD / SATD of the blocks against the
originals are the entries of intra_ref.tables: the emitted block is the one whose cost
mip_intra_device reports.  Also: the Python constants and flags mirror the header."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import intra_cases as C
import intra_ref as I
import mipgpu
import predict_ref as P
from mipgpu import layout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER = C.FILTER

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def predict_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("intra_predict") / "test_intra_predict"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "vvc-mip-gpu_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", str(exe),
                           os.path.join(REPO, "tests", "cpp", "test_intra_predict.cpp")])
    return str(exe)


@needs_gxx
@pytest.mark.parametrize("filt", (None, FILTER), ids=("orig", "1d_int"))
@pytest.mark.parametrize("size", ((136, 72), (60, 36)), ids=lambda s: "%dx%d" % s)
def test_host_blocks_equal_the_restatement_and_reproduce_the_tables(predict_exe, tmp_path, size, filt):
    w, h = size
    frames, refs, un, ref = C.case(w, h, filt)
    assert un.any() and not un.all()
    if filt is not None:
        assert refs.max() > 1023                              # the clip is exercised
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([w, h, refs.shape[0]], np.int32).tobytes())
        f.write(np.ascontiguousarray(refs, np.uint16).tobytes())
        f.write(np.ascontiguousarray(un, np.uint8).tobytes())
    r = subprocess.run([predict_exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "intra_predict: ok" in r.stdout, (r.returncode, r.stdout + r.stderr)
    raw = np.fromfile(dst, np.uint16)
    shape, x, y, bw, bh = layout.cu_geometry(w, h, np.arange(un.size))
    ok = np.nonzero(~un)[0]
    if h >= 64:                                               # all 47 shapes (36 rows hold no CU 64 high)
        assert set(shape[ok]) == set(range(layout.NUM_SHAPES))
    area = (bw[ok] * bh[ok]).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(2 * area)])        # a frame's blocks, CU index order
    assert raw.size == refs.shape[0] * start[-1]
    for f in range(refs.shape[0]):
        got = raw[f * start[-1]:(f + 1) * start[-1]]
        flat = frames[f].reshape(-1)
        for s in layout.SHAPES:
            sel = np.nonzero(shape[ok] == s.index)[0]
            k = ok[sel]
            if not k.size:
                continue
            b = [P.boundaries(refs[f], x[c], y[c], s.w, s.h)[:2] for c in k]
            top, left = np.stack([t for t, _ in b]), np.stack([l for _, l in b])
            want = I.predict(top, left, s.w, s.h)
            at = start[sel][:, None] + np.arange(2 * s.w * s.h)[None, :]
            blocks = got[at].reshape(k.size, 2, s.h, s.w)
            idx = (y[k, None, None] + np.arange(s.h)[None, :, None]).astype(np.int64) * w + x[k, None, None] + np.arange(s.w)[None, None, :]
            orig = flat[idx]
            for m in range(2):
                assert np.array_equal(blocks[:, m], want[m]), (f, s.name, m)
                assert np.array_equal(P.sad_blocks(orig, blocks[:, m]), ref["sad"][f, k, m]), (f, s.name, m)
                assert np.array_equal(P.satd_blocks(orig, blocks[:, m]), ref["satd"][f, k, m]), (f, s.name, m)


def test_python_constants_mirror_the_header():
    src = open(os.path.join(REPO, "include", "mipgpu.h")).read()
    defs = {k: int(v.rstrip("uU"), 0) for k, v in re.findall(r"^#define\s+(MIP_\w+)\s+(0x[0-9a-fA-F]+|\d+)[uU]?\b", src, flags=re.M)}
    assert defs["MIP_PRED_REGULAR"] == mipgpu.PRED_REGULAR == 1
    assert defs["MIP_MODE_PLANAR"] == mipgpu.MODE_PLANAR == I.MODE_PLANAR
    assert defs["MIP_MODE_DC"] == mipgpu.MODE_DC == I.MODE_DC
    assert defs["MIP_PRED_NONE"] == mipgpu.PRED_NONE
    assert defs["MIP_PRED_PACKED"] == mipgpu.PRED_LAYOUTS["packed"] and defs["MIP_PRED_FRAME"] == mipgpu.PRED_LAYOUTS["frame"]
    assert defs["MIP_PART_MAX_LEAVES"] == mipgpu.PART_MAX_LEAVES
    assert re.search(r"^#define\s+MIPGPU_ABI_VERSION\s+7$", src, flags=re.M)   # additive: the ABI version stays
    assert "PRED_REGULAR" in mipgpu.__all__
    # the flags entry points and the chain are declared with the issue's signatures
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert "uint32_t *d_skipped, unsigned flags, void *stream);" in text
    assert "int64_t out_samples, unsigned flags, int64_t *skipped);" in text
    assert "int mip_predicted_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes, const int32_t *penalty, const int32_t *bias," in text
    import inspect
    assert inspect.signature(mipgpu.MipEngine.predict).parameters["regular"].default is False
    assert inspect.signature(mipgpu.MipEngine.predict_device).parameters["regular"].default is False
    assert list(inspect.signature(mipgpu.MipEngine.predicted_frames).parameters) == ["self", "frames", "penalty", "bias", "refs"]
