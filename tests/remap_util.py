"""The rectifier restated in numpy, owing nothing to the kernels (k_rectify.hip) or to the oracle (lvto_init_undistort_rectify_map, lvto_remap_bilinear): the
definition is "RECTIFICATION" in include/lvt_amd_ext.h.  tests/test_remap_cases.py holds remap() to answers worked out by hand and both functions to the oracle.

rectify_maps  cv::initUndistortRectifyMap with CV_32FC1 maps: iR = (P R)^-1 by the closed-form 3 x 3 inverse, per row the homogeneous coordinate accumulated
              column by column in fp64, the Brown-Conrady polynomial (k1 k2 p1 p2 k3) in the oracle's operation order, narrowed to fp32.
remap         cv::remap, 8UC1, INTER_LINEAR, BORDER_CONSTANT 0, in integer arithmetic, for a source of any size under a map of any size; with it a
              per-pixel BRANCH CODE the tests build their coverage conditions on."""
import numpy as np

INT_MIN = -2 ** 31
# the branch of one output pixel.  An INT_MIN entry (either map) comes first, then where the 2 x 2 block lies: outside, on one of the eight partial places,
# or whole inside (the fast path) -- there all_integer where both fractions are zero (the weights 32767, 0, 0, 1)
CODES = {"fast": 0, "outside": 1, "left": 2, "right": 3, "top": 4, "bottom": 5, "top_left": 6, "top_right": 7, "bottom_left": 8, "bottom_right": 9,
         "all_integer": 10, "int_min": 11}
CODE_NAMES = {v: k for k, v in CODES.items()}
_PARTIAL = {(0, 1): 2, (0, 2): 3, (1, 0): 4, (2, 0): 5, (1, 1): 6, (1, 2): 7, (2, 1): 8, (2, 2): 9}   # (row place, column place): 1 = before the source, 2 = behind it


def to_fixed(m):
    """map entries -> 1/32-px fixed point (int64 array): cvRound(m * 32.f) where the fp32 product is finite and inside (-2^31, 2^31), INT_MIN otherwise"""
    m = np.asarray(m, np.float32)
    with np.errstate(all="ignore"):
        p = m * np.float32(32.0)                      # (an fp32 product)
        ok = np.isfinite(p) & (np.abs(p) < np.float32(2.0 ** 31))
        r = np.rint(np.where(ok, p, np.float32(0)))   # (round half to even)
    return np.where(ok, r.astype(np.int64), np.int64(INT_MIN))


def weights(ax, ay):
    """the four 15-bit weights of the fraction pair (arrays or scalars)"""
    ax, ay = np.asarray(ax, np.int64), np.asarray(ay, np.int64)
    w = [(32 - ax) * (32 - ay) * 32, ax * (32 - ay) * 32, (32 - ax) * ay * 32, ax * ay * 32]
    both = (ax == 0) & (ay == 0)        # 32768 saturates to 32767 as a short; the table's sum fix-up puts the missing 1 on the last weight
    w[0] = np.where(both, 32767, w[0])
    w[3] = np.where(both, 1, w[3])
    return w


def remap(src, map1, map2, out_pitch=None):
    """(plane, code): plane is (dh, out_pitch or dw) uint8 with zero in the padding columns, code (dh, dw) the branch of every pixel"""
    src = np.asarray(src, np.uint8)
    sh, sw = src.shape
    map1, map2 = np.asarray(map1, np.float32), np.asarray(map2, np.float32)
    assert map1.shape == map2.shape and map1.ndim == 2
    dh, dw = map1.shape
    fx, fy = to_fixed(map1), to_fixed(map2)
    sx, sy = np.clip(fx >> 5, -32768, 32767), np.clip(fy >> 5, -32768, 32767)   # (>> on a negative int64 floors)
    ax, ay = fx & 31, fy & 31                                                    # (never negative)
    w = weights(ax, ay)
    acc = np.zeros((dh, dw), np.int64)
    S = src.astype(np.int64)
    for k, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yy, xx = sy + oy, sx + ox
        inside = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw)                   # BORDER_CONSTANT: a pixel that is not there counts as 0
        acc += np.where(inside, S[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], 0) * w[k]
    val = np.clip((acc + (1 << 14)) >> 15, 0, 255)
    outside = (sx >= sw) | (sx + 1 < 0) | (sy >= sh) | (sy + 1 < 0)
    val = np.where(outside, 0, val)
    col = np.where(sx < 0, 1, np.where(sx + 1 >= sw, 2, 0))
    row = np.where(sy < 0, 1, np.where(sy + 1 >= sh, 2, 0))
    code = np.where((ax == 0) & (ay == 0), CODES["all_integer"], CODES["fast"])
    for (r, c), v in _PARTIAL.items():
        code = np.where((row == r) & (col == c), v, code)
    code = np.where(outside, CODES["outside"], code)
    code = np.where((fx == INT_MIN) | (fy == INT_MIN), CODES["int_min"], code)
    pitch = dw if out_pitch is None else int(out_pitch)
    assert pitch >= dw
    plane = np.zeros((dh, pitch), np.uint8)
    plane[:, :dw] = val.astype(np.uint8)
    return plane, code.astype(np.int8)


def rectify_maps(K, D, R, P, w, h):
    """(map1, map2), float32 (h, w)"""
    K, R, P = (np.asarray(a, np.float64).reshape(3, 3) for a in (K, R, P))
    k1, k2, p1, p2, k3 = (float(d) for d in np.asarray(D, np.float64).reshape(5))
    S = [0.0] * 9
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += float(P[i, k]) * float(R[k, j])
            S[3 * i + j] = s
    ir = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
    if d != 0.0:
        d = 1.0 / d
        ir = [(S[4] * S[8] - S[5] * S[7]) * d, (S[2] * S[7] - S[1] * S[8]) * d, (S[1] * S[5] - S[2] * S[4]) * d,
              (S[5] * S[6] - S[3] * S[8]) * d, (S[0] * S[8] - S[2] * S[6]) * d, (S[2] * S[3] - S[0] * S[5]) * d,
              (S[3] * S[7] - S[4] * S[6]) * d, (S[1] * S[6] - S[0] * S[7]) * d, (S[0] * S[4] - S[1] * S[3]) * d]
    fx, fy, u0, v0 = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    rows = np.arange(h, dtype=np.float64)

    def along_rows(step, per_row, start):
        a = np.full((h, w), step, np.float64)
        a[:, 0] = rows * per_row + start
        return np.add.accumulate(a, axis=1)      # (the same left-to-right chain of adds as _x += ir[0])
    with np.errstate(all="ignore"):
        _x, _y, _w = along_rows(ir[0], ir[1], ir[2]), along_rows(ir[3], ir[4], ir[5]), along_rows(ir[6], ir[7], ir[8])
        iw = 1.0 / _w
        x, y = _x * iw, _y * iw
        x2, y2 = x * x, y * y
        r2, _2xy = x2 + y2, 2 * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((0 * r2 + 0) * r2 + 0) * r2)
        xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + 0 * r2 + 0 * r2 * r2
        yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + 0 * r2 + 0 * r2 * r2
        u = fx * 1.0 * xd + u0
        v = fy * 1.0 * yd + v0
        return u.astype(np.float32), v.astype(np.float32)


def maps_equal(a, b):
    """a map entry is equal when both are NaN, or the bits are equal (a NaN's sign and payload are no part of the contract)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.uint32) == b.view(np.uint32))))
