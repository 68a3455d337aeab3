"""The numpy restatement of the angular intra costs (tests/angular_ref.py) pinned by
hand-checkable cases (no GPU): the pure and the exact-diagonal modes sample by sample, the two
PDPC formulas on a 4x4 and a 4x64 CU, frames every sample of which one mode predicts exactly,
ties on a uniform frame, the inverse-angle table; and the launcher's grid cap that the
multi-pass GPU test sizes its batch from."""
import time

import numpy as np
import pytest

import angular_cases as AC
import angular_ref as A
import launch_caps
import mipgpu
from mipgpu import layout

UN = layout.UNAVAILABLE


def _boundaries(w, h, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1024, (3, w)), rng.integers(0, 1024, (3, h)), rng.integers(0, 1024, 3)


@pytest.mark.parametrize("size", ((4, 4), (8, 8), (16, 4), (4, 64), (32, 8)), ids=lambda s: "%dx%d" % s)
def test_pure_and_diagonal_modes_sample_by_sample(size):
    w, h = size
    top, left, corner = _boundaries(w, h, w * 100 + h)
    p = dict(zip((2, 18, 34, 50, 66), A.predict(top, left, corner, w, h, (2, 18, 34, 50, 66), pdpc=False)))
    for n in range(3):
        for j in range(h):
            for i in range(w):
                assert p[50][n, j, i] == top[n, i] and p[18][n, j, i] == left[n, j]
                diag = top[n, i - j - 1] if i > j else corner[n] if i == j else left[n, j - i - 1]
                assert p[34][n, j, i] == diag, (i, j)
                assert p[66][n, j, i] == top[n, min(i + j + 1, w - 1)]
                assert p[2][n, j, i] == left[n, min(i + j + 1, h - 1)]


def _weight(d, scale):
    s = (2 * d) >> scale
    return 32 >> s if s <= 5 else 0


@pytest.mark.parametrize("size", ((4, 4), (4, 64)), ids=lambda s: "%dx%d" % s)
def test_pdpc_of_the_pure_modes(size):
    """m = 50: refL = left[j] - corner + top[i], weight by the column; m = 18: refT = top[i] -
    corner + left[j], weight by the row -- written out per sample.  Boundaries up to 4000 (an
    engine filter's last columns) make the clip fire on both sides."""
    w, h = size
    rng = np.random.default_rng(h)
    top, left, corner = rng.integers(0, 4001, (4, w)), rng.integers(0, 4001, (4, h)), rng.integers(0, 4001, 4)
    scale = {(4, 4): 0, (4, 64): 1}[size]
    assert scale == ((w.bit_length() - 1) + (h.bit_length() - 1) - 2) >> 2
    got = dict(zip((18, 50), A.predict(top, left, corner, w, h, (18, 50))))
    low = high = cut = False
    for n in range(4):
        for j in range(h):
            for i in range(w):
                wl, wt = _weight(i, scale), _weight(j, scale)
                cut |= wt == 0
                v50 = ((int(left[n, j]) - int(corner[n]) + int(top[n, i])) * wl + (64 - wl) * int(top[n, i]) + 32) >> 6
                v18 = ((int(top[n, i]) - int(corner[n]) + int(left[n, j])) * wt + (64 - wt) * int(left[n, j]) + 32) >> 6
                low |= v50 < 0 or v18 < 0
                high |= v50 > 1023 or v18 > 1023
                assert got[50][n, j, i] == min(max(v50, 0), 1023) and got[18][n, j, i] == min(max(v18, 0), 1023), (n, i, j)
    assert low and high
    assert cut                                                # the weight cut at shift > 5: row 3 of 4x4, rows 6.. of 4x64
    assert _weight(0, 0) == 32 and _weight(2, 0) == 2 and _weight(3, 0) == 0 and _weight(5, 1) == 1 and _weight(6, 1) == 0


@pytest.mark.parametrize("kind, mode", (("x", 50), ("y", 18), ("x-y", 34)))
def test_structured_frames_cost_nothing_in_their_mode(kind, mode):
    """f(x) is predicted exactly by mode 50 (PDPC included: left[j] == corner), f(y) by mode 18,
    f(x - y) by mode 34, on every available CU with x > 0 and y > 0.  CUs that reach past the
    right frame edge compare against the next row's samples (linear index): f(x) still matches
    there (the top row wraps the same way), f(y) and f(x - y) do not, so for those two the CUs
    are the ones inside the frame."""
    w, h = 136, 72
    frame = AC.structured(kind, w, h)
    un = mipgpu.unavailable_cus(w, h)
    tabs = A.tables(frame, frame, un, (18, 34, 50))
    _, x, y, bw, _ = layout.cu_geometry(w, h, np.arange(un.size))
    inner = ~un & (x > 0) & (y > 0)
    if kind != "x":
        inner &= x + bw <= w
    assert inner.sum() > 1000
    for key in AC.TABLES:
        assert not tabs[key][inner, mode - 2].any(), key
    am, ac = A.best(tabs["cost"])
    assert np.all(am[inner] == 0x80 + mode) and not ac[inner].any()
    others = [m for m in (18, 34, 50) if m != mode]
    assert all(tabs["cost"][inner, m - 2].min() > 0 for m in others)


def test_uniform_frame_ties_go_to_the_first_mode_of_the_list():
    w, h = 136, 72
    frame = np.full((h, w), 700, np.uint16)
    un = mipgpu.unavailable_cus(w, h)
    for modes in (None, (7, 30, 61), (66,)):
        tabs = A.tables(frame, frame, un, modes)
        listed = np.zeros(65, bool)
        listed[np.array(A.ALL_MODES if modes is None else modes) - 2] = True
        cost = tabs["cost"]
        assert np.all(cost[:, ~listed] == UN) and np.all(cost[un] == UN)
        assert np.all(cost[~un][:, listed] == cost[~un][:, listed][:, :1])          # every listed mode ties
        am, ac = A.best(cost)
        first = 2 if modes is None else modes[0]
        assert np.all(am[~un] == 0x80 + first) and np.all(am[un] == 0xFF) and np.all(ac[un] == UN)
    _, x, y, _, _ = layout.cu_geometry(w, h, np.arange(un.size))
    assert not ac[~un & (x > 0) & (y > 0)].any()


def test_merge_rule():
    mode = np.array([3, 3, 3, 0xFF, 0xF0, 3], np.uint8)
    cost = np.array([100, 100, 100, UN, 50, 100], np.int32)
    am = np.array([0x82, 0x82, 0x82, 0x82, 0xC2, 0xFF], np.uint8)
    ac = np.array([90, 95, 96, 10, 44, UN], np.int32)
    m, c = A.merge(mode, cost, am, ac, 5)
    assert m.tolist() == [0x82, 3, 3, 0xFF, 0xC2, 3]          # 95 lower, 100 ties and stays, 101 higher
    assert c.tolist() == [95, 100, 100, UN, 49, 100]


def test_angle_and_inverse_tables():
    assert sorted(A.ANGLE) == list(range(2, 67))
    assert [A.ANGLE[m] for m in (2, 18, 19, 34, 35, 50, 51, 66)] == [32, 0, -1, -32, -29, 0, 1, 32]
    for m in range(2, 67):
        assert A.ANGLE[m] == A.ANGLE[68 - m]                    # the two classes mirror at mode 34
        a = abs(A.ANGLE[m])
        if a:
            assert A.INVERSE[a] == int(16384 / a + 0.5)
    assert all(A.ANGLE[m] > A.ANGLE[m + 1] for m in range(2, 34)) and all(A.ANGLE[m] < A.ANGLE[m + 1] for m in range(34, 66))
    assert mipgpu.MODE_ANGULAR_BASE == A.MODE_BASE == 0x80 and mipgpu.ANGULAR_MODES == A.MODES == 65
    codes = {A.MODE_BASE + m for m in range(2, 67)}
    assert min(codes) == 0x82 and max(codes) == 0xC2 and not codes & {mipgpu.MODE_PLANAR, mipgpu.MODE_DC, 0xFF}
    assert min(codes) >= 2 * max(s.modes for s in layout.SHAPES)


def test_one_cu_equals_the_tables_and_the_restatement_is_quick():
    """cu_costs (one CU, any size) agrees with the vectorised tables; the all-modes tables of the
    three 136x72 frames take well under a minute."""
    w, h = 136, 72
    t0 = time.perf_counter()
    frames, refs, un, ref = AC.case(w, h, None)
    assert time.perf_counter() - t0 < 60
    shape, x, y, bw, bh = layout.cu_geometry(w, h, np.arange(un.size))
    rng = np.random.default_rng(9)
    for k in rng.choice(np.nonzero(~un)[0], 12, replace=False):
        sad, satd, cost = A.cu_costs(frames[1], refs[1], x[k], y[k], bw[k], bh[k])
        assert np.array_equal(sad, ref["sad"][1, k]) and np.array_equal(satd, ref["satd"][1, k]) and np.array_equal(cost, ref["cost"][1, k])
    assert np.array_equal(ref["cost"], np.where(ref["sad"] == UN, UN, np.minimum(2 * ref["sad"].astype(np.int64), ref["satd"])))


def test_launch_cap_matches_the_launcher():
    """launch_angular caps its grid at ANGULAR_ITEMS_PER_CU workgroups per CU over the intra
    kernel's items (the multi-pass GPU test sizes its batch from it): the shared launch rule and item
    walk of launch_caps.WINDOW_HEADER, which launcher and kernel go through."""
    assert launch_caps.uses_window_rules("mip_angular.hip", "launch_angular", "angular_kernel")
    body = launch_caps.launcher_body(launch_caps.WINDOW_HEADER, "launch_window_kernel")
    caps = launch_caps.CAP_EXPRESSION.findall(body)
    assert caps == [(str(AC.ANGULAR_ITEMS_PER_CU),) * 2], caps
    assert "a.nframes * a.nctus * kItemsPerCtu" in body
    kernel = launch_caps.kernel_body("mip_angular.hip", "angular_kernel")
    text = launch_caps.window_text()
    assert "g += gridDim.x" in kernel and text.count("const bool big = k < %d;" % AC.ANGULAR_BIG_ITEMS) == 1
    assert text.count("constexpr int kItemsPerCtu = 4 + kIntraBlocks;") == 1 and AC.ANGULAR_ITEMS_PER_CTU == 20
