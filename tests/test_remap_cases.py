"""CPU tier: the numpy restatement of the rectifier (remap_util) against answers worked out by hand, against the oracle on every planted case and
calibration (remap_cases), and the conditions on those inputs that make them worth running: every branch, every weight pair, every kind of tie, and a
calibration whose map really holds NaN, infinities and entries beyond 2^26.  The GPU tier (test_gpu_rectifier_edges.py) holds the kernels to the same
restatement."""
import numpy as np
import pytest

import remap_cases as RC
import remap_util as RU

NAN, INF = float("nan"), float("inf")
S3 = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.uint8)
U2 = np.array([[255, 0], [0, 255]], np.uint8)
X6 = np.full((5, 6), 50, np.uint8)
X6[0, 0] = 255

# (source, mx, my, value, branch): every value below was computed by hand from the definition -- the sum of value x weight, + 16384, >> 15
BY_HAND = [
    # fixed point (16, 8): corner (0, 0), fractions 16 and 8; weights 12288 12288 4096 4096 on 10 20 40 50: 737280 + 16384 = 753664 = 23 x 32768
    (S3, 0.5, 0.25, 23, "fast"),
    # corner (1, 1), both fractions zero: 50 x 32767 + 90 x 1 + 16384 = 1654824 -> 50
    (S3, 1.0, 1.0, 50, "all_integer"),
    (S3, 3.0, 1.0, 0, "outside"),                  # corner column 3 == sw
    (S3, -1.5, 1.0, 0, "outside"),                 # fixed point -48 >> 5 = -2: the floor, not -1
    # fixed point -16: corner column -1 (the floor), fraction 16; weights 16384 16384 0 0 on (0, 10): 163840 + 16384 = 180224 -> 5
    (S3, -0.5, 0.0, 5, "left"),
    # fixed point 72: column 2, fraction 8; row 1: weights 24576 8192 on (60, 0): 1474560 + 16384 = 1490944 -> 45
    (S3, 2.25, 1.0, 45, "right"),
    # fixed point -8 in y: row -1, fraction 24; weights 8192 . 24576 . on (0, ., 20, .): 491520 + 16384 = 507904 -> 15
    (S3, 1.0, -0.25, 15, "top"),
    # row 2, fraction 16: weight 16384 on 70: 1146880 + 16384 = 1163264 -> 35
    (S3, 0.0, 2.5, 35, "bottom"),
    # both -16: only the last weight, 16 x 16 x 32 = 8192, meets a pixel (10): 81920 + 16384 = 98304 = 3 x 32768
    (S3, -0.5, -0.5, 3, "top_left"),
    # column 2 fraction 0, row -1 fraction 16: weight 32 x 16 x 32 = 16384 on 30: 491520 + 16384 = 507904 -> 15
    (S3, 2.0, -0.5, 15, "top_right"),
    # column -1 fraction 24, row 2 fraction 0: weight 24 x 32 x 32 = 24576 on 70: 1720320 + 16384 = 1736704 = 53 x 32768
    (S3, -0.25, 2.0, 53, "bottom_left"),
    # column 2, row 2, fractions 16, 16: weight 8192 on 90: 737280 + 16384 = 753664 -> 23
    (S3, 2.5, 2.5, 23, "bottom_right"),
    # ties, on (255, 0 / 0, 255).  0.5 -> 0 (even): all-integer, 255 x 32767 + 255 x 1 = 255 x 32768 -> 255 (rounded up to 1: 255 x 31744 + 16384 -> 247)
    (U2, 1 / 64, 0.0, 255, "all_integer"),
    # 1.5 -> 2 (even): weights 30720 2048: 255 x 30720 + 16384 = 7849984 -> 239 (rounded down to 1: 247)
    (U2, 3 / 64, 0.0, 239, "fast"),
    # -0.5 -> -0, which is 0 (even): 255 as above (rounded away to -1: column -1, fraction 31: 255 x 31744 + 16384 -> 247)
    (U2, -1 / 64, 0.0, 255, "all_integer"),
    # -1.5 -> -2 (even): column -1, fraction 30: weight 30 x 32 x 32 = 30720 on 255 -> 239 (rounded up to -1: 247)
    (U2, -3 / 64, 0.0, 239, "left"),
    # integer_255.  A 1 x 1 source: the only pixel is the corner, its weight 32767: 255 x 32767 + 16384 = 8371969 -> 255 (without the + 16384: 254)
    (np.array([[255]], np.uint8), 0.0, 0.0, 255, "bottom_right"),
    # 254 under 32767 at the last column: 254 x 32767 + 16384 = 8339202 -> 254
    (np.array([[255, 254], [1, 255]], np.uint8), 1.0, 0.0, 254, "right"),
    # extreme: the entry is INT_MIN, the sample at -32768: 0, where pixel (0, 0) holds 255
    (X6, NAN, 0.0, 0, "int_min"),
    (X6, 0.0, INF, 0, "int_min"),
    (X6, 2.0 ** 27, 0.0, 0, "int_min"),      # (x 32 = 2^32, which wraps to 0 in a 32-bit conversion)
    (X6, -2.0 ** 26, 0.0, 0, "int_min"),     # (x 32 = -2^31: the interval is open)
    (X6, 2.0 ** 26 - 4, 0.0, 0, "outside"),  # the float below 2^26: x 32 = 2^31 - 128, a finite fixed-point value, clamped to column 32767
    (X6, 0.0, 0.0, 255, "all_integer"),      # (and the pixel the wrapped entries used to sample)
]


@pytest.mark.parametrize("k", range(len(BY_HAND)))
def test_the_restatement_gives_the_hand_computed_answer(k):
    src, mx, my, value, branch = BY_HAND[k]
    plane, code = RU.remap(src, np.array([[mx]], np.float32), np.array([[my]], np.float32), out_pitch=4)
    assert plane.shape == (1, 4) and not plane[0, 1:].any(), "the padding columns are not zero"
    assert (int(plane[0, 0]), RU.CODE_NAMES[int(code[0, 0])]) == (value, branch)


def test_to_fixed_by_hand():
    m = np.array([0.5, 1 / 64, 3 / 64, -1 / 64, -3 / 64, -1.5, 32767.96875, 2.0 ** 26 - 4, 2.0 ** 26, -2.0 ** 26, NAN, INF, -INF, 3e38], np.float32)
    want = [16, 0, 2, 0, -2, -48, 1048575, 2 ** 31 - 128] + [RU.INT_MIN] * 6
    assert RU.to_fixed(m).tolist() == want
    w = RU.weights(np.array([0, 16, 31, 0]), np.array([0, 8, 31, 1]))
    assert [[int(a[k]) for a in w] for k in range(4)] == [[32767, 0, 0, 1], [12288, 12288, 4096, 4096], [32, 992, 992, 30752], [31744, 0, 1024, 0]]


# ---- the restatement equals the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_remap_equals_the_oracle(oracle_lib, name):
    src, m1, m2 = RC.CASES[name]
    want, _ = RU.remap(src, m1, m2)
    got = oracle_lib.remap_bilinear(src, m1, m2)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{name}: {len(bad)} pixels differ, first at {tuple(bad[0])}: oracle {got[tuple(bad[0])]} numpy {want[tuple(bad[0])]}"


@pytest.mark.parametrize("name", sorted(RC.CALIBRATIONS))
def test_rectify_maps_equal_the_oracle(oracle_lib, name):
    K, D, R, P, w, h = RC.CALIBRATIONS[name]
    mine, theirs = RU.rectify_maps(K, D, R, P, w, h), oracle_lib.init_undistort_rectify_map(K, D, R, P, w, h)
    for k in (0, 1):
        assert mine[k].shape == (h, w) and mine[k].dtype == np.float32
        assert RU.maps_equal(mine[k], theirs[k]), f"{name}: map{k + 1} differs"


def test_the_old_wrap_is_gone_from_the_oracle(oracle_lib):
    """with the oracle alone: every planted pixel of `extreme` is 0.  ((int)lrintf wrapped modulo 2^32: NaN, the infinities and every entry from 2^27 upward
    sampled source pixel (0, 0), which holds 255 here.)"""
    src, m1, m2 = RC.CASES["extreme/6x5"]
    assert src[0, 0] == 255 and (np.delete(src.reshape(-1), 0) < 100).all()
    got = oracle_lib.remap_bilinear(src, m1, m2).reshape(-1)[:RC.EXTREME_PLANTED]
    bad = [(float(m1.reshape(-1)[k]), float(m2.reshape(-1)[k]), int(got[k])) for k in np.flatnonzero(got)]
    assert not bad, f"(mx, my, pixel): {bad}"


# ---- coverage, as a condition on the inputs (the restatement alone) -------------------------------------------------------------------------------
def branch_counts():
    """{case: {branch: pixels}}"""
    out = {}
    for name, (src, m1, m2) in sorted(RC.CASES.items()):
        code = RU.remap(src, m1, m2)[1]
        out[name] = {RU.CODE_NAMES[int(c)]: int(n) for c, n in zip(*np.unique(code, return_counts=True))}
    return out


def test_every_branch_and_every_weight_pair_occurs():
    seen, pairs = set(), set()
    for name, counts in branch_counts().items():
        seen |= set(counts)
    for src, m1, m2 in RC.CASES.values():
        fx, fy = RU.to_fixed(m1), RU.to_fixed(m2)
        live = (fx != RU.INT_MIN) & (fy != RU.INT_MIN)
        pairs |= set(zip((fx[live] & 31).tolist(), (fy[live] & 31).tolist()))
    assert seen == set(RU.CODES), set(RU.CODES) - seen
    assert len(pairs) == 1024
    # the groups hold what their names say
    per_group = {g: set().union(*(set(c) for n, c in branch_counts().items() if n.startswith(g + "/"))) for g in RC.GROUPS}
    assert {"left", "right", "top", "bottom", "top_left", "top_right", "bottom_left", "bottom_right", "outside"} <= per_group["edges"]
    assert "all_integer" in per_group["integer_255"] and "int_min" in per_group["extreme"]
    for n, c in branch_counts().items():
        if n.startswith("thin_sources/") and not n.endswith("2x2"):
            assert "fast" not in c and "all_integer" not in c, (n, c)       # max(sw - 1, 0) == 0 or max(sh - 1, 0) == 0: no pixel takes the fast path
    assert set(RC.GROUPS) == {"ties", "negative", "edges", "integer_255", "fractions", "clamp", "extreme", "thin_sources", "narrow_outputs", "zoom"}


def test_both_tie_parities_occur_with_either_sign():
    for axis in (0, 1):
        seen = set()
        for name, case in RC.CASES.items():
            if name.startswith("ties/"):
                p = case[1 + axis].astype(np.float64) * 32          # (exact: the entries are small multiples of 1/64)
                tie = p - np.floor(p) == 0.5
                seen |= set(zip((np.floor(p[tie]) % 2 == 0).tolist(), (p[tie] < 0).tolist()))
        assert seen == {(True, True), (True, False), (False, True), (False, False)}, (axis, seen)
    # a tie rounds to the even neighbour: k + 0.5 -> k for even k, k + 1 for odd k
    k = np.array(RC._TIE_K)
    assert RU.to_fixed(((2 * k + 1) / 64.0).astype(np.float32)).tolist() == np.where(k % 2 == 0, k, k + 1).tolist()


def test_the_last_weight_of_the_all_integer_entry_cannot_show_in_eight_bits():
    """why no case tells the weights 32767, 0, 0, 1 from 32767, 0, 0, 0 (or from an unsaturated 32768): v0 x 32767 + v3 w3 + 16384 = v0 x 32768 + (16384 - v0 +
    v3 w3), and the bracket stays inside 0 ... 32767 for 8-bit values, so the pixel is v0 whatever w3 is.  What integer_255 does catch is the entry together
    with a wrong rounding term: 255 x 32767 >> 15 is 254"""
    v0, v3 = np.meshgrid(np.arange(256), np.arange(256))
    for w0, w3 in ((32767, 1), (32767, 0), (32768, 0)):
        assert np.array_equal((v0 * w0 + v3 * w3 + (1 << 14)) >> 15, v0)
    assert (255 * 32767) >> 15 == 254


def test_negative_entries_carry_every_fraction():
    fx = RU.to_fixed(RC.CASES["negative/x"][1])
    neg = fx[fx < 0]
    assert set((neg & 31).tolist()) == set(range(32)) and set((neg >> 5).tolist()) == {-1, -2}


def test_the_clamp_case_reaches_the_clamp_where_it_shows():
    """on the 32770-wide source an unclamped corner column of 32768 or 32769 is a pixel of the source: only the clamp keeps it at 32767"""
    for name, axis in (("clamp/wide_source", 0), ("clamp/high_source", 1)):
        src, m1, m2 = RC.CASES[name]
        coarse = RU.to_fixed((m1, m2)[axis]) >> 5
        assert ((coarse > 32767) & (coarse < max(src.shape))).sum() >= 3
    fx = RU.to_fixed(RC.CASES["clamp/small"][1])
    assert (fx >> 5).max() > 32767 and (fx >> 5).min() < -32768 and 32767 in (fx >> 5) and -32768 in (fx >> 5)


def test_the_calibrations_reach_what_they_are_named_for():
    m = np.stack(RU.rectify_maps(*RC.CALIBRATIONS["horizon_in_image"]))
    finite = np.isfinite(m)
    assert np.isnan(m).any() and np.isinf(m).any() and (np.abs(m[finite]) > 2.0 ** 26).any() and (np.abs(m[finite]) < 64).any()
    K, D, R, P, w, h = RC.CALIBRATIONS["zoom_out_4x"]
    code = RU.remap(np.zeros((h, w), np.uint8), *RU.rectify_maps(K, D, R, P, w, h))[1]
    assert np.mean(code == RU.CODES["outside"]) > 0.5
    m1, m2 = RU.rectify_maps(*RC.CALIBRATIONS["singular_P"])     # ir is the identity: (x, y) = (column, row), unnormalised
    K, D = RC.CALIBRATIONS["singular_P"][:2]
    assert m1[0, 0] == np.float32(K[2]) and m2[0, 0] == np.float32(K[5]) and m1[0, 1] > 30
    m1, m2 = RU.rectify_maps(*RC.CALIBRATIONS["identity"])
    assert np.array_equal(m1, np.tile(np.arange(40, dtype=np.float32), (24, 1))) and np.array_equal(m2, np.tile(np.arange(24, dtype=np.float32)[:, None], (1, 40)))
    m1, _ = RU.rectify_maps(*RC.CALIBRATIONS["shift_by_1_5_px"])
    assert np.array_equal(m1, np.tile(np.arange(40, dtype=np.float32) - 1.5, (24, 1)))
    assert set(RC.CALIBRATIONS) == {"identity", "shift_by_1_5_px", "barrel", "barrel_2x", "pincushion", "pincushion_2x", "tangential_only", "rotated_10deg",
                                    "rotated_30deg", "horizon_in_image", "singular_P", "zoom_out_4x", "one_pixel", "one_row", "one_column"}
    assert [RC.CALIBRATIONS[n][4:] for n in ("one_pixel", "one_row", "one_column")] == [(1, 1), (65, 1), (1, 65)]
