"""Depth guard: the numpy restatement of the rule (include/lvt_amd_ext.h, DEPTH GUARD) per pixel and per feature list, the records the tests use, and the route
by which the unchanged oracle tracks a guarded frame.  No expected value comes from the library under test.

THE RULE.  A pixel's sample s is the fp32 value itself, or float32(raw) * float32(scale) for a 16-bit plane (one rounded multiply).  valid(s) is
near <= s <= far (a NaN is not valid).  For every feature the gather step kept, in its output order, with (bx, by) the raw position:
    cx = (int)bx;  cy = (int)by                   -- truncation; inside the plane when bx > -1 && bx < W && by > -1 && by < H
    d_c = s(cx, cy);  dropped when the pixel is outside the plane or d_c is not valid
    t = tol_abs + tol_rel * d_c                   -- a rounded fp32 multiply, then a rounded fp32 add
    support = #{(dx, dy) != (0, 0), |dx|, |dy| <= radius, (cx + dx, cy + dy) inside the plane : valid(s) and |s - d_c| <= t}   -- a rounded fp32 subtract
    keep = support >= min_support
Every operand below is float32 and the multiply, the add and the subtract are separate numpy operations, so the results are the kernel's bit for bit.

THE EQUIVALENCE.  Detected corners are integers, so a guarded frame equals Oracle.track_rgbd(gray, guarded_depth(depth)): a zero depth fails the near-plane
test (near_plane > 0) exactly where the guard drops, and the low-corner retry does not look at depth."""
from collections import namedtuple

import numpy as np

Guard = namedtuple("Guard", "radius min_support tol_abs tol_rel")
DEFAULT = Guard(1, 4, 0.01, 0.02)       # lvt_amd_depth_guard_default
STRICT = Guard(1, 6, 0.01, 0.02)        # the record of the sequence tests: drops the key points that sit on a layer edge


def samples(depth, scale=None):
    """the fp32 samples of a plane: itself (float32), or float32(raw) * float32(scale) (uint16)"""
    d = np.asarray(depth)
    if d.dtype == np.uint16:
        assert scale is not None
        s = d.astype(np.float32) * np.float32(scale)
    else:
        assert d.dtype == np.float32, d.dtype
        s = d
    assert s.dtype == np.float32
    return s


def valid(s, near, far):
    with np.errstate(invalid="ignore"):
        return (np.float32(near) <= s) & (s <= np.float32(far))


def support_plane(depth, cfg, near, far, scale=None):
    """per pixel: the support its sample has in its window (int32, (H, W)); meaningful where the sample itself is valid"""
    s = samples(depth, scale)
    H, W = s.shape
    r = int(cfg.radius)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = np.float32(cfg.tol_rel) * s
        t = np.float32(cfg.tol_abs) + prod
        assert prod.dtype == np.float32 and t.dtype == np.float32
        padded = np.full((H + 2 * r, W + 2 * r), np.nan, np.float32)   # (outside the plane: not valid, which is what the clipped window says)
        padded[r:r + H, r:r + W] = s
        support = np.zeros((H, W), np.int32)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dx == 0 and dy == 0:
                    continue
                nb = padded[r + dy:r + dy + H, r + dx:r + dx + W]
                diff = nb - s
                assert diff.dtype == np.float32
                support += (valid(nb, near, far) & (np.abs(diff) <= t)).astype(np.int32)
    return support


def keep_plane(depth, cfg, near, far, scale=None):
    """bool (H, W): a key point on this pixel is kept"""
    return valid(samples(depth, scale), near, far) & (support_plane(depth, cfg, near, far, scale) >= int(cfg.min_support))


def guarded_depth(depth, cfg, near, far, scale=None):
    """where(valid & support >= min_support, depth, 0), in the plane's own element type"""
    depth = np.asarray(depth)
    assert float(near) > 0.0, "a zero must fail the near-plane test"
    return np.where(keep_plane(depth, cfg, near, far, scale), depth, np.zeros_like(depth)).astype(depth.dtype)


def keep_features(bx, by, depth, cfg, near, far, scale=None):
    """bool array: the rule on a feature list's fp32 raw positions (any bit pattern) against the plane"""
    kp = keep_plane(depth, cfg, near, far, scale)
    H, W = kp.shape
    fx, fy = np.asarray(bx, dtype=np.float32).ravel(), np.asarray(by, dtype=np.float32).ravel()
    with np.errstate(invalid="ignore"):
        inside = (fx > np.float32(-1)) & (fx < np.float32(W)) & (fy > np.float32(-1)) & (fy < np.float32(H))
    keep = np.zeros(fx.shape, dtype=bool)
    cx, cy = np.trunc(fx[inside]).astype(np.int64), np.trunc(fy[inside]).astype(np.int64)
    keep[inside] = kp[cy, cx]
    return keep


def compact(arrays, keep):
    """the stage entry's result for the eight arrays: (count, the kept elements of each in order)"""
    return int(keep.sum()), [np.asarray(a).ravel()[keep] for a in arrays]


def features_of(corners, depth, near, far, W, H, B=28, scale=None):
    """the detector's corners that are features of the UNGUARDED frame: behind BRIEF's border filter (cvRound, 28 px) and with a valid depth sample"""
    xyr = np.asarray(corners)
    ix, iy = np.rint(xyr[:, 0]).astype(np.int64), np.rint(xyr[:, 1]).astype(np.int64)
    inside = (ix >= B) & (ix < W - B) & (iy >= B) & (iy < H - B)
    xyr, ix, iy = xyr[inside], ix[inside], iy[inside]
    return xyr[valid(samples(depth, scale)[iy, ix], near, far)]


def dropped_share(corners, depth, cfg, near, far, what, at_least=0.0, scale=None):
    """(dropped, share of the DETECTOR's corners): the unguarded frame's features among `corners` that the guard drops, counted against every corner the
    detector found; asserts that the guard drops at least one, and at least `at_least` of the detector's corners"""
    depth = np.asarray(depth)
    H, W = depth.shape
    feats = features_of(corners, depth, near, far, W, H, scale=scale)
    n = len(feats)
    k = int(keep_features(feats[:, 0], feats[:, 1], depth, cfg, near, far, scale).sum()) if n else 0
    assert n > 0 and k < n, f"{what}: the guard drops none of the {n} features -- the case compares nothing"
    share = (n - k) / len(corners)
    assert share >= at_least, f"{what}: the guard drops {share:.1%} of the detector's {len(corners)} corners, the case needs {at_least:.0%}"
    return n - k, share
