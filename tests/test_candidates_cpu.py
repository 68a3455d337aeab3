"""K-best candidate lists on the CPU (no GPU): the numpy restatement tests/candidates_ref.py pinned
on CUs that can be checked by hand -- a three-way tie across the families, fewer candidates than
k, no candidate, a bias that moves the winner, absent MIP entries -- and against the existing
merges' restatements at k = 1; the synthetic tables of the GPU test really hold what that test is
about; the launcher's grid rule as tests/test_gpu_candidates.py assumes it; and the kernel's
build-time resources."""
import os
import re

import numpy as np

import angular_ref as A
import candidates_ref as C
import intra_ref as I
import kernel_resources
import launch_caps as L

UN = C.UN
LIB = os.path.join(os.path.dirname(__file__), "..", "vvc-mip-gpu_amd", "lib", "libmipgpu.so")


def _ang(**slots):
    row = np.full(65, UN, np.int32)
    for m, v in slots.items():
        row[int(m[1:]) - 2] = v
    return row


def test_hand_checked_cus():
    # CU 0: MIP 7, Planar and angular 2 tie at 4 -> MIP, Planar, angular; then DC 5, MIP 2 at 9
    # CU 1: two candidates only (a MIP mode above 31 and an UNAVAILABLE entry are absent)
    # CU 2: none
    # CU 3: angular 50 at 10 against MIP 0 at 10: the MIP mode wins the tie; DC at 10 is between
    mip_mode = np.array([[7, 2, 0xFF], [40, 5, 9], [0xFF, 0xFF, 0xFF], [0, 0xFF, 0xFF]], np.uint8)
    mip_cost = np.array([[4, 9, UN], [0, 6, UN], [UN, UN, UN], [10, UN, UN]], np.int32)
    intra = np.array([[4, 5], [UN, UN], [UN, UN], [11, 10]], np.int32)
    ang = np.stack([_ang(m2=4), _ang(m66=6), _ang(), _ang(m50=10, m18=12)])
    modes, costs = C.candidates(5, mip_mode, mip_cost, intra, None, ang, 0)
    assert modes.tolist() == [[7, 0xF0, 0x82, 0xF1, 2], [5, 0x80 + 66, 0xFF, 0xFF, 0xFF], [0xFF] * 5, [0, 0xF1, 0x80 + 50, 0xF0, 0x80 + 18]]
    assert costs.tolist() == [[4, 4, 4, 5, 9], [6, 6, UN, UN, UN], [UN] * 5, [10, 10, 10, 11, 12]]
    assert C.count(mip_mode, mip_cost, intra, ang).tolist() == [5, 2, 0, 5]
    # k = 1 and k = 2 are prefixes
    for k in (1, 2):
        m, c = C.candidates(k, mip_mode, mip_cost, intra, None, ang, 0)
        assert np.array_equal(m, modes[:, :k]) and np.array_equal(c, costs[:, :k])
    # biases move the winners and are part of the values: CU 0 with Planar + 1 and angular + 2
    m, c = C.candidates(3, mip_mode, mip_cost, intra, (1, 0), ang, 2)
    assert m[0].tolist() == [7, 0xF0, 0xF1] and c[0].tolist() == [4, 5, 5]
    assert m[3].tolist() == [0, 0xF1, 0xF0] and c[3].tolist() == [10, 10, 12]
    m, c = C.candidates(2, mip_mode, mip_cost, intra, (0, 3), ang, 0)
    assert m[3].tolist() == [0, 0x80 + 50] and c[3].tolist() == [10, 10]
    # families alone
    m, c = C.candidates(2, ang_cost=ang)
    assert m.tolist() == [[0x82, 0xFF], [0x80 + 66, 0xFF], [0xFF, 0xFF], [0x80 + 50, 0x80 + 18]]
    m, c = C.candidates(2, intra_cost=intra, intra_bias=(2, 0))
    assert m.tolist() == [[0xF1, 0xF0], [0xFF, 0xFF], [0xFF, 0xFF], [0xF1, 0xF0]] and c[0].tolist() == [5, 6]
    m, c = C.candidates(3, mip_mode, mip_cost)
    assert m.tolist() == [[7, 2, 0xFF], [5, 0xFF, 0xFF], [0xFF] * 3, [0, 0xFF, 0xFF]]


def test_top_of_the_domain():
    ang = np.stack([_ang(m2=C.TOP, m3=8380416, m66=0), _ang(m34=C.TOP)])
    intra = np.array([[C.TOP, 0], [8380416, C.TOP]], np.int32)
    m, c = C.candidates(5, intra_cost=intra, intra_bias=(C.MAX_BIAS, C.MAX_BIAS), ang_cost=ang, ang_bias=C.MAX_BIAS)
    assert m[0].tolist() == [0xF1, 0x80 + 66, 0x83, 0xF0, 0x82]
    assert c[0].tolist() == [1 << 20, 1 << 20, 8380416 + (1 << 20), (1 << 24) - 1, (1 << 24) - 1]
    assert m[1].tolist() == [0xF0, 0xF1, 0x80 + 34, 0xFF, 0xFF] and c[1, 2] == (1 << 24) - 1 and c[1, 3] == UN


def test_column_0_is_what_the_existing_merges_leave():
    """k = 1 against the merges' own restatements (tests/intra_ref.py, tests/angular_ref.py) on
    random tables with many ties: search argmin -> Planar / DC merge -> angular merge."""
    rng = np.random.default_rng(11)
    ncu = 4000
    best_cost = rng.integers(0, 6, (1, ncu)).astype(np.int32)
    best_mode = rng.integers(0, 32, (1, ncu)).astype(np.uint8)
    intra = rng.integers(0, 6, (1, ncu, 2)).astype(np.int32)
    ang = rng.integers(0, 6, (1, ncu, 65)).astype(np.int32)
    ang[rng.random(ang.shape) < 0.6] = UN
    dead = rng.random((1, ncu)) < 0.05
    best_cost[dead], best_mode[dead], intra[dead], ang[dead] = UN, 0xFF, UN, UN
    for bias, ab in (((0, 0), 0), ((1, 2), 1)):
        mode, cost = I.merge(best_mode, best_cost, intra, bias)
        am, ac = A.best(ang)
        mode, cost = A.merge(mode, cost, am, ac, ab)
        m, c = C.candidates(1, best_mode[..., None], best_cost[..., None], intra, bias, ang, ab)
        assert np.array_equal(m[..., 0], mode) and np.array_equal(c[..., 0], cost)
        assert (mode >= 0x82).any() and (mode < 32).any() and (mode == 0xF0).any() and (mode == 0xF1).any() and (mode == 0xFF).any()


def test_synthetic_tables_hold_what_the_gpu_test_is_about():
    for kin in (1, 3, 32):
        t = C.synthetic(5380 * 2, kin, kin)
        n = C.count(t["mip_mode"], t["mip_cost"], t["intra_cost"], t["ang_cost"])
        assert (n == 0).any() and ((n > 0) & (n < 3)).any() and (n > 32).any()
        assert 0.02 < (n == 0).mean() < 0.09
        alive = np.stack([C.count(t["mip_mode"], t["mip_cost"]) > 0, C.count(intra_cost=t["intra_cost"]) > 0, C.count(ang_cost=t["ang_cost"]) > 0])
        for fam in range(3):
            assert (alive[fam] & (alive.sum(axis=0) == 1)).any(), fam         # CUs with this family alone
        assert ((t["mip_mode"] > 31) & (t["mip_mode"] != 0xFF)).any() and (t["mip_mode"] == 0xFF).any()
        m, c = C.candidates(3, **t)
        fam_of = np.where(m < 32, 0, np.where(m >= 0xF0, 1, 2))
        tie = (c[:, 0] == c[:, 1]) & (c[:, 0] != UN) & (fam_of[:, 0] != fam_of[:, 1])
        assert tie.mean() > 0.2                                                # cross-family ties are the rule
        v = C.rows(len(m), **t)
        for cu in np.nonzero(n > 0)[0][:50]:                                  # distinct MIP modes: nothing is lost
            assert (v[cu] != C.ABSENT).sum() == n[cu]


def test_the_launcher_takes_one_lane_per_cu():
    """tests/test_gpu_candidates.py sizes its ragged launch from this: one workgroup of 64 lanes per
    64 CUs, no cap, the last workgroup short."""
    text = L.launcher_body("mip_candidates.hip", "launch_candidates")
    with open(os.path.join(L.CSRC, "mip_candidates.hip")) as f:
        source = f.read()
    assert re.search(r"constexpr int kCandLanes = 64;", source)
    assert re.search(r"grid\s*=\s*\(a\.total_cus \+ kCandLanes - 1\) / kCandLanes;", text)
    assert "dim3((unsigned)grid), dim3(kCandLanes)" in text
    body = L.kernel_body("mip_candidates.hip", "candidates_kernel")
    assert "__syncthreads" not in body and "blockIdx.x * kCandLanes" in body       # every lane works on its own row only
    assert 5380 % 64 == 4                                     # a CTU is 84 workgroups and four CUs


def test_the_kernel_has_no_scratch():
    assert os.path.exists(LIB), "libmipgpu.so is not built"
    found = {n: k for n, k in kernel_resources.kernels(LIB).items() if "candidates_kernel" in n}
    assert len(found) == 1
    (k,) = found.values()
    assert k[".private_segment_fixed_size"] == 0
    assert k[".vgpr_count"] <= 64 and k[".group_segment_fixed_size"] == 0      # 8 waves per SIMD; LDS is sized by the launch
