"""Feature masks, the CPU tier: the numpy restatement of the rule (mask_util.keep_rule) on hand-written cases, and the facts about the unchanged oracle that the
GPU tier (test_gpu_feature_masks.py) rests on -- the three masks' drop shares, that the oracle tracks every frame under each of them through the routes the
equivalences name, that its detector's coordinates are integers on these worlds, and what a frame without corners does to it.

The worlds: the KITTI-shaped world 71 at 621 x 187 (stereo) and the TUM-shaped world 0 at 322 x 242 (RGB-D), 8 frames each."""
import numpy as np
import pytest

import mask_util as MU
from parity_util import make_case

KITTI, TUM = ("kitti", 71, (621, 187)), ("tum", 0, (322, 242))


# ---- the restatement on hand-written cases -----------------------------------------------------------------------------------------------------
def one(x, y, mask):
    return bool(MU.keep_rule([x], [y], mask)[0])


def only(W, H, x, y, v=255):
    m = np.zeros((H, W), np.uint8)
    m[y, x] = v
    return m


def test_half_belongs_to_the_next_pixel():
    """k + 0.5 + 0.5f is k + 1 exactly: truncation lands on pixel k + 1, in x and in y"""
    for k in (0, 3, 10):
        assert one(k + 0.5, 2.0, only(16, 8, k + 1, 2)) and not one(k + 0.5, 2.0, only(16, 8, k, 2))
        assert one(2.0, k % 6 + 0.5, only(16, 8, 2, k % 6 + 1)) and not one(2.0, k % 6 + 0.5, only(16, 8, 2, k % 6))
    assert one(3.25, 2.0, only(16, 8, 3, 2)) and one(3.75, 2.0, only(16, 8, 4, 2))


def test_the_fp32_add_rounds_up_below_a_half():
    """0.49999997 is the float below 0.5; 0.49999997f + 0.5f = 1 - 2^-25 is a tie between 1 - 2^-24 and 1 and rounds to even: pixel 1, where real
    arithmetic (and a double-precision add) says pixel 0"""
    c = np.float32(0.49999997)
    assert c < np.float32(0.5) and c + MU.HALF == np.float32(1.0) and int(float(c) + 0.5) == 0
    assert one(c, c, only(8, 8, 1, 1)) and not one(c, c, only(8, 8, 0, 0))


def test_negative_coordinates():
    """truncation is toward zero: every sum in (-1, 0) is pixel 0 (OpenCV's own behaviour), a sum of -1 or less is outside"""
    m = only(8, 8, 0, 0)
    assert one(-0.4, -0.4, m) and one(-0.7, 0.0, m) and one(0.0, -1.4, m)
    assert not one(-1.5, 0.0, m) and not one(0.0, -1.5, m) and not one(-3.0, -3.0, np.full((8, 8), 255, np.uint8))
    assert not one(np.nan, 0.0, np.full((8, 8), 255, np.uint8))


def test_the_last_column_and_row():
    W, H = 12, 7
    full = np.full((H, W), 255, np.uint8)
    assert one(W - 1, H - 1, only(W, H, W - 1, H - 1))
    assert one(W - 0.75, 0, only(W, H, W - 1, 0))            # (W - 0.25 truncates to W - 1)
    assert not one(W - 0.5, 0, full) and not one(W, 0, full) and not one(W + 5, 0, full)
    assert not one(0, H - 0.5, full) and not one(0, H, full) and one(0, H - 0.75, only(W, H, 0, H - 1))


def test_any_non_zero_byte_keeps():
    for v in (1, 7, 128, 255):
        assert one(4, 4, only(8, 8, 4, 4, v))
    assert not one(4, 4, np.zeros((8, 8), np.uint8))
    assert one(4, 4, only(8, 8, 4, 4).astype(bool))


def test_an_empty_list_and_the_order():
    m = MU.checkerboard(64, 48, cell=4, value=1)
    assert MU.keep_rule(np.zeros(0, np.float32), np.zeros(0, np.float32), m).shape == (0,)
    assert MU.filter_corners(np.zeros((0, 3), np.float32), m).shape == (0, 3)
    rng = np.random.default_rng(5)
    xyr = np.stack([rng.uniform(-2, 66, 500), rng.uniform(-2, 50, 500), np.arange(500)], axis=1).astype(np.float32)
    kept = MU.filter_corners(xyr, m)
    assert 0 < len(kept) < 500 and np.all(np.diff(kept[:, 2]) > 0), "the filter keeps the order"


# ---- the masks and the oracle ---------------------------------------------------------------------------------------------------------------
class World:
    def __init__(self, kind, seed, size, n=8):
        from oracle import pyoracle as O
        self.world, self.prm, self.sensor = make_case(kind, seed, 1.0, None, size)
        self.W, self.H = size
        if self.sensor == 1:
            self.frames = [tuple(np.ascontiguousarray(a) for a in self.world.render_stereo(i)) for i in range(n)]
            self.corners = [tuple(O.detect_grid(a, self.prm)[0] for a in f) for f in self.frames]
        else:
            self.frames = [tuple(np.ascontiguousarray(a) for a in self.world.render_rgbd(i)) for i in range(n)]
            self.corners = [(O.detect_grid(f[0], self.prm)[0],) for f in self.frames]


_W = {}


def world_of(case):
    if case not in _W:
        _W[case] = World(*case)
    return _W[case]


def shares(w, mask, eyes, features=False):
    out = []
    for c in w.corners:
        for e in eyes:
            x = MU.border_kept(c[e], w.W, w.H) if features else c[e]
            out.append(1.0 - float(MU.keep_rule(x[:, 0], x[:, 1], mask).mean()))
    return min(out), max(out)


def test_the_detectors_coordinates_are_integers(oracle_lib):
    """what the RGB-D equivalence rests on: a corner IS the pixel its depth is read at, so zeroing the depth under the mask is the mask"""
    for case in (KITTI, TUM):
        for c in world_of(case).corners:
            for xyr in c:
                assert len(xyr) > 200 and np.array_equal(xyr[:, :2], np.rint(xyr[:, :2])) and xyr[:, :2].min() >= 0


# (mask, eyes the range is stated for, lowest and highest share of the detector's corners dropped in a frame, lowest and highest match count of frames 1 .. 7)
KITTI_FIGURES = [("bonnet", (0, 1), 0.26, 0.32, 160, 198), ("checkerboard", (0, 1), 0.45, 0.53, 37, 61), ("ellipse", (0,), 0.25, 0.28, 186, 211)]


@pytest.mark.parametrize("name,eyes,lo,hi,m_lo,m_hi", KITTI_FIGURES, ids=[f[0] for f in KITTI_FIGURES])
def test_kitti_shaped_world_under_the_masks(oracle_lib, name, eyes, lo, hi, m_lo, m_hi):
    """the oracle tracks all 8 frames through the external-corner route; the mask drops the stated share of the detector's corners in every frame, at
    least one FEATURE (a corner behind the border filter) in every frame and eye, and at least 10 % of them for the bonnet and the checkerboard"""
    w = world_of(KITTI)
    mask = MU.MASKS[name](w.W, w.H)
    got = shares(w, mask, eyes)
    print(name, "corners dropped", got, "features dropped", shares(w, mask, (0, 1), True))
    assert lo <= got[0] and got[1] <= hi + 0.005, got   # (the figures are whole per cent: half a point of rounding)
    assert shares(w, mask, (0, 1), True)[0] > max(MU.MIN_SHARE[name], 0.0)
    orc, matches = oracle_lib.Oracle(w.prm, 1), []
    for i, (L, R) in enumerate(w.frames):
        MU.oracle_track_masked(orc, w.prm, L, R, mask, mask, f"{name} frame {i}", MU.MIN_SHARE[name])
        assert orc.status == 2, f"{name}: the oracle is not TRACKING at frame {i}"
        matches.append(orc.counts()["n_matches"])
    print(name, "matches", matches)
    assert m_lo <= min(matches[1:]) and max(matches[1:]) <= m_hi, matches


@pytest.mark.parametrize("name", list(MU.MASKS))
def test_tum_shaped_world_under_the_masks(oracle_lib, name):
    """the oracle tracks all 8 frames with the depth zeroed under the mask.  Of its FEATURES the ellipse drops 3 - 6 % here (its half axes reach past the
    border filter's frame except in the corners), the bonnet and the checkerboard far more than the 10 % their cases need"""
    w = world_of(TUM)
    mask = MU.MASKS[name](w.W, w.H)
    got = shares(w, mask, (0,), True)
    print(name, "features dropped", got)
    assert got[0] > max(MU.MIN_SHARE[name], 0.0)
    if name == "ellipse":
        assert 0.03 <= got[0] and got[1] <= 0.06, got
    orc = oracle_lib.Oracle(w.prm, 2)
    for i, (g, d) in enumerate(w.frames):
        orc.track_rgbd(g, MU.masked_depth(d, mask))
        assert orc.status == 2, f"{name}: the oracle is not TRACKING at frame {i}"


def test_a_frame_without_corners_loses_the_oracle_for_good(oracle_lib):
    w = world_of(KITTI)
    orc, none = oracle_lib.Oracle(w.prm, 1), np.zeros((0, 2))
    states = []
    for i, (L, R) in enumerate(w.frames[:6]):
        if i == 2:
            orc.track_with_external_corners(L, R, none, none)
        else:
            MU.oracle_track_masked(orc, w.prm, L, R, None, None)
        states.append(orc.status)
    assert states == [2, 2, 3, 3, 3, 3], states
