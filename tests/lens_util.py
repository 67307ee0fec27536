"""The lens models restated in numpy, owing nothing to the kernels (k_rectify_map_radtan, k_rectify_map_fisheye): the definition is "LENS MODELS" in
include/lvt_amd_ext.h.  The row chains are the np.add.accumulate chains of remap_util.rectify_maps (the same left-to-right adds as _x += iR[0]).

lens_maps_f64   (u, v) in fp64, before the float cast -- what the round-trip tests read
lens_maps       (map1, map2), float32 (dh, dw)
project         a model's own FORWARD formula: a ray (x, y, 1) of the raw camera -> the raw pixel (the direction a camera model is usually written in)"""
import numpy as np

RADTAN, FISHEYE = 0, 1


def inverse_PR(R, P):
    """iR = (P R)^-1 as 9 Python floats: the product summed over k ascending, the inverse by cofactors; the identity where the determinant is 0"""
    R, P = (np.asarray(a, np.float64).reshape(3, 3) for a in (R, P))
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
    return ir


def _coeffs(D, n):
    D = np.asarray(D, np.float64).reshape(-1)
    assert D.size <= 12
    return [float(d) for d in np.concatenate([D, np.zeros(12 - D.size)])[:n]]


def lens_maps_f64(model, K, D, R, P, dw, dh, atan=np.arctan):
    """(u, v), float64 (dh, dw).  `atan`: the arctangent FISHEYE uses (the tests perturb it to bound what its last bits can move)"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, u0, v0 = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    ir = inverse_PR(R, P)
    rows = np.arange(dh, dtype=np.float64)

    def along_rows(step, per_row, start):
        a = np.full((dh, dw), step, np.float64)
        a[:, 0] = rows * per_row + start
        return np.add.accumulate(a, axis=1)      # (the same left-to-right chain of adds as _x += ir[0])
    with np.errstate(all="ignore"):
        _x, _y, _w = along_rows(ir[0], ir[1], ir[2]), along_rows(ir[3], ir[4], ir[5]), along_rows(ir[6], ir[7], ir[8])
        if model == RADTAN:
            k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _coeffs(D, 12)
            iw = 1.0 / _w
            x, y = _x * iw, _y * iw
            x2, y2 = x * x, y * y
            r2, _2xy = x2 + y2, 2 * x * y
            kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
            xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2
            yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2
            return fx * xd + u0, fy * yd + v0
        assert model == FISHEYE
        k1, k2, k3, k4 = _coeffs(D, 4)
        behind = _w <= 0
        x, y = _x / _w, _y / _w
        r = np.sqrt(x * x + y * y)
        theta = atan(r)
        t2 = theta * theta
        t4 = t2 * t2
        t6, t8 = t4 * t2, t4 * t4
        theta_d = theta * (1 + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8)
        scale = np.where(r == 0, 1.0, theta_d / r)
        u, v = fx * x * scale + u0, fy * y * scale + v0
        u = np.where(behind, np.where(_x > 0, -np.inf, np.inf), u)
        v = np.where(behind, np.where(_y > 0, -np.inf, np.inf), v)
        return u, v


def lens_maps(model, K, D, R, P, dw, dh, atan=np.arctan):
    """(map1, map2), float32 (dh, dw)"""
    with np.errstate(all="ignore"):
        u, v = lens_maps_f64(model, K, D, R, P, dw, dh, atan)
        return u.astype(np.float32), v.astype(np.float32)


def project(model, K, D, x, y):
    """the raw pixel (u, v) of the ray (x, y, 1) in the raw camera's frame: the model's forward formula, in plain fp64"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, u0, v0 = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    if model == RADTAN:
        k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _coeffs(D, 12)
        r2 = x * x + y * y
        kr = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r2 ** 2
        yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r2 ** 2
        return fx * xd + u0, fy * yd + v0
    k1, k2, k3, k4 = _coeffs(D, 4)
    r = float(np.hypot(x, y))
    if r == 0.0:
        return u0, v0
    th = float(np.arctan(r))
    th_d = th * (1 + k1 * th ** 2 + k2 * th ** 4 + k3 * th ** 6 + k4 * th ** 8)
    return fx * x * th_d / r + u0, fy * y * th_d / r + v0


def outside_fraction(map1, map2, sw, sh):
    """the share of map entries that fall outside a sw x sh source (NaN and infinities count as outside)"""
    with np.errstate(all="ignore"):
        inside = (map1 >= 0) & (map1 <= sw - 1) & (map2 >= 0) & (map2 <= sh - 1)
    return 1.0 - float(np.mean(inside))


def ulp_distance(a, b):
    """per entry, how many fp32 values lie between a and b (finite entries): the distance of their ordered integer images"""
    def ordered(f):
        i = np.ascontiguousarray(f, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))
