"""Phase A's clipping conversion (mip_search.hip convert_pair), modelled in numpy.

The MFMA delivers x = (D + beta) / 1024 for the unclipped reduced sample D, a multiple of 1/64;
v_cvt_pknorm_u16_f32 turns x into the u16 x * 65535, saturating at 0 and 65535, and a packed
shift right by 6 must leave clip(floor(D), 0, 1023).  The instruction's rounding is not
documented, so the model runs every variant the hardware probe admits: tools/pknorm_probe.hip on
an MI355X (profiles/pknorm_probe.txt) found beta = 2^-7 exact and beta = 2^-6 not, which rules a
truncating conversion out (it would need 2^-6, shown below) and leaves the round-to-nearest
family -- ties to even, ties up, add 0.5 and truncate -- with the product x * 65535 taken exactly
or rounded to f32 first.  The kernel's beta must be exact under all six.

Range: every D = j / 64 with |D| < 2^16 + 1024 (|D| < 2^16 is the kernel's bound, phase_a)."""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCH = os.path.join(REPO, "vvc-mip-gpu_amd", "csrc", "mip_search.hip")
J = np.arange(-64 * (2 ** 16 + 1024) + 1, 64 * (2 ** 16 + 1024), dtype=np.int64)  # D = J / 64
WANT = np.clip(J >> 6, 0, 1023)


def _kernel_beta():
    """kPredBeta and kPredScale as mip_search.hip states them."""
    m = re.search(r"constexpr float kPredBeta = 1\.0f / (\d+)\.0f, kPredScale = 1\.0f / (\d+)\.0f;", open(SEARCH).read())
    assert m, "kPredBeta / kPredScale not found in mip_search.hip"
    assert int(m.group(2)) == 1024
    return 1.0 / int(m.group(1))


ROUNDINGS = {
    "nearest-even": np.rint,
    "half-up": lambda p: np.floor(p + 0.5),
    "add-half-truncate": lambda p: np.trunc(p + 0.5),
    "truncate": np.trunc,
}


def _convert(beta, rounding, f32_product):
    x = ((J + 64 * beta) / 65536.0).astype(np.float32)  # (D + beta) / 1024
    assert np.array_equal(x.astype(np.float64) * 65536.0, J + 64 * beta), "x is not exact in f32"
    p = x.astype(np.float64) * 65535.0                   # exact: 24 x 16 bits
    if f32_product:
        p = p.astype(np.float32).astype(np.float64)
    u = np.where(x <= 0, 0.0, np.where(x >= 1, 65535.0, ROUNDINGS[rounding](p)))
    return u.astype(np.int64) >> 6


@pytest.mark.parametrize("f32_product", [False, True], ids=["exact-product", "f32-product"])
@pytest.mark.parametrize("rounding", ["nearest-even", "half-up", "add-half-truncate"])
def test_kernel_beta_is_exact_under_every_admitted_rounding(rounding, f32_product):
    beta = _kernel_beta()
    assert beta == 2.0 ** -7  # what the probe found exact
    bad = int((_convert(beta, rounding, f32_product) != WANT).sum())
    print("beta 2^-7, %s, %s: %d mismatches of %d" % (rounding, "f32" if f32_product else "exact", bad, J.size))
    assert bad == 0


def test_the_probe_tells_the_roundings_apart():
    """Why the probe's two betas decide the rounding: a truncating conversion is exact with
    2^-6 and not with 2^-7; the nearest family is the other way round."""
    for f32_product in (False, True):
        assert int((_convert(2.0 ** -6, "truncate", f32_product) != WANT).sum()) == 0
        assert int((_convert(2.0 ** -7, "truncate", f32_product) != WANT).sum()) > 0
        for rounding in ("nearest-even", "half-up", "add-half-truncate"):
            assert int((_convert(2.0 ** -6, rounding, f32_product) != WANT).sum()) > 0


def test_scaled_accumulator_rows_are_exact(tmp_path):
    """The kernel prologue rewrites the tables' f32 C rows as (c + beta) * 2^-10 (scaled_c): for
    every entry of build_tables()'s C region that is exact in f32 -- the sum and the product."""
    exe = tmp_path / "dump_tables"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "vvc-mip-gpu_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", str(exe),
                           os.path.join(REPO, "tests", "cpp", "dump_tables.cpp")])
    raw = subprocess.run([str(exe)], capture_output=True, check=True, timeout=60).stdout
    weight_bytes, ctab_rows = 768 * 16, 384 + 4  # mip_work.h kWeightRows, kCtabRows
    assert len(raw) == weight_bytes + ctab_rows * 4
    c = np.frombuffer(raw[weight_bytes:], np.float32)
    assert np.isfinite(c).all() and (c[384:] == 0.5 - 1024.0).all()
    beta = np.float32(_kernel_beta())
    s32 = c + beta                              # f32 arithmetic, as the kernel's
    assert np.array_equal(s32.astype(np.float64), c.astype(np.float64) + float(beta))
    y32 = s32 * np.float32(2.0 ** -10)
    assert np.array_equal(y32.astype(np.float64), (c.astype(np.float64) + float(beta)) / 1024.0)
    # and the values are on the grid the exactness argument assumes: C' a multiple of 1/64
    assert np.array_equal(np.rint(c.astype(np.float64) * 64), c.astype(np.float64) * 64)
