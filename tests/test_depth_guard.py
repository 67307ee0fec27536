"""Depth guard, the CPU tier: the numpy restatement of the rule (depth_guard_util) on hand-written planes with known answers, against a scalar walk of the
definition, and the facts about the unchanged oracle that the GPU tier (test_gpu_depth_guard.py) rests on -- that it tracks every frame of the TUM-shaped world
0 at 322 x 242 on the guarded plane, and how many of its detector's corners the two records drop there."""
import numpy as np
import pytest

import depth_guard_util as DG
from parity_util import make_case

NEAR, FAR = 0.1, 5.0
R1 = DG.Guard(1, 4, 0.01, 0.02)
f32 = np.float32


def support(plane, x, y, cfg=R1, scale=None):
    return int(DG.support_plane(plane, cfg, NEAR, FAR, scale)[y, x])


def kept(plane, x, y, cfg=R1, scale=None):
    return bool(DG.keep_plane(plane, cfg, NEAR, FAR, scale)[y, x])


def scalar_support(s, x, y, cfg, near=NEAR, far=FAR):
    """the definition walked pixel by pixel with float32 scalars: None where the centre is not valid"""
    H, W = s.shape
    ok = lambda v: bool(f32(near) <= v) and bool(v <= f32(far))
    d_c = s[y, x]
    if not ok(d_c):
        return None
    with np.errstate(invalid="ignore", over="ignore"):
        t = f32(cfg.tol_abs) + f32(f32(cfg.tol_rel) * d_c)
        n = 0
        for dy in range(-cfg.radius, cfg.radius + 1):
            for dx in range(-cfg.radius, cfg.radius + 1):
                px, py = x + dx, y + dy
                if (dx or dy) and 0 <= px < W and 0 <= py < H and ok(s[py, px]) and bool(np.abs(f32(s[py, px] - d_c)) <= t):
                    n += 1
    return n


# ---- hand-written planes ------------------------------------------------------------------------------------------------------------------------
def test_a_straight_step_edge():
    """foreground 1 m left of column 6, background 3 m: a foreground pixel on the edge has its own column and the one behind it, 5 of 8"""
    p = np.full((9, 12), 3.0, f32)
    p[:, :6] = 1.0
    assert support(p, 5, 4) == 5 and support(p, 6, 4) == 5 and support(p, 4, 4) == 8 and support(p, 7, 4) == 8
    assert kept(p, 5, 4) and not kept(p, 5, 4, DG.STRICT) and kept(p, 4, 4, DG.STRICT)


def test_a_convex_corner_tip():
    """the tip of a foreground rectangle: 3 of 8; the background pixel diagonally outside it sees 7"""
    p = np.full((9, 12), 3.0, f32)
    p[:5, :6] = 1.0
    assert support(p, 5, 4) == 3 and support(p, 6, 5) == 7
    assert not kept(p, 5, 4) and kept(p, 6, 5, DG.STRICT)


def test_a_flying_column():
    """one column of in-between depths: its pixels support one another along the column only, 2 of 8"""
    p = np.full((9, 12), 3.0, f32)
    p[:, :6] = 1.0
    p[:, 6] = 2.0
    assert support(p, 6, 4) == 2 and not kept(p, 6, 4)
    assert support(p, 5, 4) == 5 and support(p, 7, 4) == 5


def test_a_lone_valid_pixel_in_a_hole():
    p = np.zeros((9, 12), f32)
    p[4, 6] = 2.0
    assert support(p, 6, 4) == 0 and not kept(p, 6, 4, DG.Guard(1, 1, 0.01, 0.02))
    assert not DG.keep_plane(p, DG.Guard(3, 1, 10.0, 10.0), NEAR, FAR).any(), "a zero is not valid however wide the tolerance"


def test_neighbours_that_are_nan_inf_or_zero():
    p = np.full((5, 5), 2.0, f32)
    p[1, 1], p[1, 2], p[1, 3], p[2, 1] = np.nan, np.inf, 0.0, -np.inf
    assert support(p, 2, 2) == 4 and kept(p, 2, 2) and not kept(p, 2, 2, DG.Guard(1, 5, 0.01, 0.02))
    for x, y in ((1, 1), (2, 1), (3, 1), (1, 2)):
        assert not kept(p, x, y, DG.Guard(1, 1, 0.01, 0.02)), "an invalid centre is dropped"
    assert not kept(np.full((5, 5), -0.0, f32), 2, 2, DG.Guard(1, 1, 1.0, 1.0))


def test_a_sample_exactly_t_away_and_its_fp32_neighbours():
    """t = 0.125 + 0.0625 * 2 = 0.25 exactly: 2.25 and the float below it count, the float above does not; likewise on the near side"""
    cfg = DG.Guard(1, 1, 0.125, 0.0625)
    for s, want in ((f32(2.25), 1), (np.nextafter(f32(2.25), f32(0)), 1), (np.nextafter(f32(2.25), f32(9)), 0),
                    (f32(1.75), 1), (np.nextafter(f32(1.75), f32(9)), 1), (np.nextafter(f32(1.75), f32(0)), 0)):
        p = np.zeros((3, 3), f32)
        p[1, 1], p[0, 2] = 2.0, s
        assert support(p, 1, 1, cfg) == want, (s, want)


def test_the_tolerance_is_two_rounded_fp32_operations():
    """0.01f + 0.02f * 3.7f in float32 differs from the double-precision value rounded once; the restatement uses the former"""
    d = f32(3.7)
    t32 = f32(0.01) + f32(f32(0.02) * d)
    p = np.zeros((3, 3), f32)
    p[1, 1] = d
    p[1, 2] = d + t32          # (exact or rounded: what matters is that plane and scalar walk agree)
    cfg = DG.Guard(1, 1, 0.01, 0.02)
    assert support(p, 1, 1, cfg) == scalar_support(p, 1, 1, cfg)
    assert t32.dtype == np.float32


def test_the_window_is_clipped_at_the_border():
    p = np.full((9, 12), 2.0, f32)
    for r, corner, edge, inner in ((1, 3, 5, 8), (2, 8, 14, 24), (3, 15, 27, 48)):
        cfg = DG.Guard(r, 1, 0.01, 0.02)
        assert (support(p, 0, 0, cfg), support(p, 11, 8, cfg), support(p, 5, 0, cfg), support(p, 0, 4, cfg)) == (corner, corner, edge, edge)
        assert support(p, 5, 4, cfg) == inner


def test_16_bit_raws_with_a_scale():
    """the sample is float32(raw) * float32(scale), one rounded multiply: the guard of a raw plane is the guard of its converted plane"""
    scale = f32(1.0 / 5000.0)
    raw = np.full((9, 12), 15000, np.uint16)
    raw[:, :6] = 5000
    raw[:, 6] = 10000
    raw[0, 0] = 0            # no depth
    raw[8, 11] = 65535       # 13.1 m: behind the far plane
    conv = raw.astype(np.float32) * scale
    assert np.array_equal(DG.samples(raw, scale), conv)
    for cfg in (R1, DG.STRICT, DG.Guard(2, 10, 0.01, 0.02)):
        assert np.array_equal(DG.support_plane(raw, cfg, NEAR, FAR, scale), DG.support_plane(conv, cfg, NEAR, FAR))
        g = DG.guarded_depth(raw, cfg, NEAR, FAR, scale)
        assert g.dtype == np.uint16 and np.array_equal(g != 0, DG.keep_plane(conv, cfg, NEAR, FAR))
    assert support(raw, 6, 4, scale=scale) == 2 and not kept(raw, 0, 0, DG.Guard(1, 1, 9.0, 9.0), scale) and not kept(raw, 11, 8, DG.Guard(1, 1, 9.0, 9.0), scale)
    assert support(raw, 1, 1, scale=scale) == 7, "the hole at (0, 0) is no support"


def test_the_plane_form_equals_a_scalar_walk():
    rng = np.random.default_rng(11)
    p = rng.choice(np.array([0.0, 0.09999999, 0.1, 1.0, 1.01, 1.02, 1.03, 1.05, 2.0, 2.05, 4.9999995, 5.0, 5.0000005, np.nan, np.inf, -1.0], f32), size=(13, 17))
    for cfg in (R1, DG.Guard(2, 7, 0.01, 0.02), DG.Guard(3, 20, 0.03, 0.0), DG.Guard(1, 8, 0.0, 0.05)):
        sp, kp = DG.support_plane(p, cfg, NEAR, FAR), DG.keep_plane(p, cfg, NEAR, FAR)
        for y in range(13):
            for x in range(17):
                want = scalar_support(p, x, y, cfg)
                assert bool(kp[y, x]) == (want is not None and want >= cfg.min_support), (x, y, cfg)
                assert want is None or sp[y, x] == want, (x, y, cfg)


def test_the_feature_list_form():
    """truncation toward zero, the range decided on the float, any bit pattern; the order is kept"""
    p = np.zeros((5, 7), f32)
    p[0:3, 0:3] = 2.0
    cfg = DG.Guard(1, 3, 0.01, 0.02)
    bx = np.array([0.0, -0.9, 0.99, 1.5, -1.0, 7.0, 6.5, np.nan, 1.0, np.inf, 1.0], f32)
    by = np.array([0.0, -0.5, 0.2, 1.9, 0.0, 0.0, 4.5, 1.0, np.nan, 1.0, -np.inf], f32)
    assert DG.keep_features(bx, by, p, cfg, NEAR, FAR).tolist() == [True, True, True, True, False, False, False, False, False, False, False]
    n, (a,) = DG.compact([np.arange(11)], DG.keep_features(bx, by, p, cfg, NEAR, FAR))
    assert n == 4 and a.tolist() == [0, 1, 2, 3]
    assert DG.keep_features(np.zeros(0, f32), np.zeros(0, f32), p, cfg, NEAR, FAR).shape == (0,)


# ---- the oracle on the guarded plane ---------------------------------------------------------------------------------------------------------------
class World:
    def __init__(self, n=8):
        from oracle import pyoracle as O
        self.world, self.prm, self.sensor = make_case("tum", 0, 1.0, None, (322, 242))
        self.near, self.far = self.prm.near_plane_distance, self.prm.far_plane_distance
        self.frames = [tuple(np.ascontiguousarray(a) for a in self.world.render_rgbd(i)) for i in range(n)]
        self.corners = [O.detect_grid(g, self.prm)[0] for g, _ in self.frames]


_W = []


def the_world():
    if not _W:
        _W.append(World())
    return _W[0]


def test_the_detectors_coordinates_are_integers(oracle_lib):
    """what the equivalence rests on: a corner IS the pixel its depth is read at, so zeroing the depth where the guard drops is the guard"""
    w = the_world()
    assert w.near > 0
    for c in w.corners:
        assert len(c) > 200 and np.array_equal(c[:, :2], np.rint(c[:, :2])) and c[:, :2].min() >= 0


def test_the_oracle_tracks_under_the_strict_record(oracle_lib):
    """{1, 6, 0.01, 0.02}: TRACKING on every frame, and at least 10 % of the detector's corners dropped on every frame (51 - 58 of its 420 - 460 corners,
    11.8 - 13.3 %; of the 311 - 333 that are features of the unguarded frame, 16 - 18 %)"""
    w = the_world()
    orc, dropped, nfeat = oracle_lib.Oracle(w.prm, 2), [], []
    for i, (g, d) in enumerate(w.frames):
        n, share = DG.dropped_share(w.corners[i], d, DG.STRICT, w.near, w.far, f"frame {i}", 0.10)
        dropped.append(n)
        orc.track_rgbd(g, DG.guarded_depth(d, DG.STRICT, w.near, w.far))
        assert orc.status == 2, f"the oracle is not TRACKING at frame {i}"
        nfeat.append(len(orc.features(0)[0]))
        assert nfeat[-1] == len(DG.features_of(w.corners[i], d, w.near, w.far, 322, 242)) - n, "the guarded plane costs the oracle exactly the dropped features"
    print("dropped", dropped, "features left", nfeat)
    assert 51 <= min(dropped) and max(dropped) <= 58, dropped


def test_the_default_record_drops_a_feature_per_frame(oracle_lib):
    """{1, 4, 0.01, 0.02}: 2 - 4 features per frame, the tips of the layers' corners; TRACKING throughout"""
    w = the_world()
    orc, dropped = oracle_lib.Oracle(w.prm, 2), []
    for i, (g, d) in enumerate(w.frames):
        dropped.append(DG.dropped_share(w.corners[i], d, DG.DEFAULT, w.near, w.far, f"frame {i}")[0])
        orc.track_rgbd(g, DG.guarded_depth(d, DG.DEFAULT, w.near, w.far))
        assert orc.status == 2, f"the oracle is not TRACKING at frame {i}"
    print("dropped", dropped)
    assert min(dropped) >= 1 and max(dropped) <= 4, dropped
