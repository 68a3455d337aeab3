"""The partial-CTU residue sweep (tests/size_sweep.py) on the CPU: the C oracle against the
reference's own kernels compiled for the host at every size of families A and B (at residues
other than 0, 32 and 64 nothing else ties the oracle to the reference), and the product's
model of the unavailable CUs (mip_unavailable_cus: work_plan.h filter_poison / reads_poison /
cu_defined) against the oracle's at every sweep size with every filter."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import size_sweep as S
from mipgpu import FILTERS, layout, unavailable_cus
from mipgpu.synth import synth_frame

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(REPO, "oracle", "_ref")
RUNNER = os.path.join(REF, "ref_cpu_runner")

needs_ref_cpu = pytest.mark.skipif(
    not (os.path.exists(RUNNER) and all(os.path.exists(os.path.join(REF, "intra_cpu_s%d.so" % s)) for s in range(3))),
    reason="reference-on-CPU libraries not built (make -C oracle ref-cpu, needs /root/reference)")


def test_every_residue_once_per_axis():
    """Families A and B: each of the 31 nonzero residues 4..124 occurs exactly once as W % 128
    and once as H % 128; A is 2x2 CTUs, B one CTU column narrower than 128; C has residue 0 on
    exactly one axis.  The literal tables are the formula's."""
    want = list(range(4, 128, 4))
    for fam in (S.FAMILY_A, S.FAMILY_B):
        assert len(fam) == 31
        assert sorted(w % 128 for w, _ in fam) == want
        assert sorted(h % 128 for _, h in fam) == want
    assert all(128 < w < 256 and 128 < h < 256 for w, h in S.FAMILY_A)
    assert all(w < 128 and h < 256 for w, h in S.FAMILY_B)
    assert any(w < 68 for w, _ in S.FAMILY_B) and any(h > 128 for _, h in S.FAMILY_B)
    rs = [(4 * i, 4 * ((7 * i) % 31 + 1)) for i in range(1, 32)]
    assert S.FAMILY_A == [(128 + r, 128 + s) for r, s in rs]
    assert S.FAMILY_B == [(r, s if i % 2 else 128 + s) for i, (r, s) in enumerate(rs, 1)]
    assert S.FAMILY_C == [(256, 128 + s) for s in (4, 28, 100, 124)] + [(128 + r, 256) for r in (4, 60, 68, 124)]
    assert all((w % 128 == 0) != (h % 128 == 0) for w, h in S.FAMILY_C)
    assert len(set(S.ALL_SIZES)) == len(S.ALL_SIZES) == 70
    # every H % 32 residue, which the filters' tile bands and the poison model depend on
    assert {h % 32 for _, h in S.ALL_SIZES} == set(range(0, 32, 4))


def test_contents_are_ten_bit_and_as_described():
    w, h = 136, 188
    for kind in S.CONTENTS:
        f = S.content(kind, w, h)
        assert f.dtype == np.uint16 and f.shape == (h, w) and f.max() <= 1023, kind
    noise, edges = S.content("noise", w, h), S.content("edges", w, h)
    assert np.array_equal(noise, synth_frame(w, h, S.seed_of(w, h), 1))
    assert (edges[:, :4] == 1023).all() and (edges[:, -4:] == 1023).all()
    assert np.array_equal(edges[:, 4:-4], noise[:, 4:-4])
    assert S.content("dark", w, h).max() == 2 and (S.content("white", w, h) == 1023).all()
    r = S.caller_refs(w, h)
    assert r[:, :-2].max() <= 1023 and r[:, -2:].min() >= 1024 and r[:, -2:].max() <= 1705
    assert S.caller_refs(256, 132).max() <= 1023


@needs_ref_cpu
@pytest.mark.parametrize("size", S.FAMILY_A + S.FAMILY_B, ids=S.size_id)
def test_oracle_equals_reference_kernels_on_cpu(tmp_path, size):
    """The reference's kernels on the host CPU (original references, uniform noise) against
    O.search on every entry the reference defines (layout.available_mask); on the complement
    the oracle says UNAVAILABLE."""
    w, h = size
    seed = S.seed_of(w, h)
    out = tmp_path / "cost.bin"
    r = subprocess.run([RUNNER, "--libs", REF, "--width", str(w), "--height", str(h), "--frames", "1",
                        "--synth", "1:%x" % seed, "--workers", str(min(8, os.cpu_count() or 1)), "--out-cost", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    cpf = layout.num_ctus(w, h) * layout.COSTS_PER_CTU
    got = np.fromfile(out, "<i4")
    assert got.size == cpf
    want = O.search(synth_frame(w, h, seed, 1))
    mask = layout.available_mask(w, h).reshape(-1)
    assert mask.any()
    bad = np.nonzero((got != want) & mask)[0]
    assert bad.size == 0, (size, bad[:5], got[bad[:5]], want[bad[:5]])
    assert (want[~mask] == layout.UNAVAILABLE).all()
    assert (want[mask] != layout.UNAVAILABLE).all()


@pytest.mark.parametrize("size", S.ALL_SIZES, ids=S.size_id)
@pytest.mark.parametrize("filt", [None] + list(FILTERS))
def test_unavailable_cus_match_the_oracle_model(size, filt):
    """As tests/test_unavailable.py, at every sweep size."""
    w, h = size
    frame = S.content("noise", w, h)
    n = layout.num_ctus(w, h)
    got = layout.expand_cu_mask(unavailable_cus(w, h, filt), n)
    assert np.array_equal(got, O.engine_unavailable_mask(frame, filt, 0)), (w, h, filt)
    # never more than the reference leaves undefined (poison + race + geometry)
    if filt is not None:
        _, und = O.filter_frame(frame, filt, 0, with_undefined=True)
        assert not (got & O.defined_mask(w, h, und)).any()
