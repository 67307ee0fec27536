"""Pose uncertainty (lvt_amd_pose_info, include/lvt_amd_ext.h): the reference the tests hold the kernel to, and the comparisons.

reference() is a numpy float64 restatement of the definition, written from the definition and not from the kernel:
  pose (R, p) camera-to-world, perturbation xi = (dp on world axes, dtheta on camera axes: R <- R Exp([dtheta]x));
  pc = R^T (X - p);  e = (fx pcx / pcz + cx - u, fy pcy / pcz + cy - v);  inlier iff pcz > 0 and e.e <= 5.991 (false for NaN);
  w = 1 / (1 + e.e / 5.991);  J = de/dpc [ -R^T | [pc]x ];  info = sum over inliers of w J^T J;  cov = inv(info)."""
import numpy as np

TH2 = 5.991
BORDER = 1e-6
PIVOT_REL = 1e-12
INFO_TOL, COV_TOL, IDENT_TOL = 1e-10, 1e-9, 1e-9


def quat_to_R(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])


def exp_so3(v):
    """Rodrigues"""
    a = float(np.linalg.norm(v))
    if a < 1e-300:
        return np.eye(3)
    K = skew(np.asarray(v, np.float64) / a)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def log_so3(R):
    """rotation vector of a rotation near the identity"""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = float(np.linalg.norm(v))
    if s < 1e-300:
        return v
    return v * (np.arcsin(min(s, 1.0)) / s)


def intrinsics_of(prm):
    """fx, fy, cx, cy as the library holds them: lvt_amd_params carries them as 32-bit floats (718.856 is 718.85601806640625 there)"""
    return tuple(float(np.float32(v)) for v in (prm.fx, prm.fy, prm.cx, prm.cy))


def project(prm, R, p, X):
    """(n, 2) pixels and the camera-frame points of world points X under the pose (R, p)"""
    fx, fy, cx, cy = intrinsics_of(prm)
    pc = (np.asarray(X, np.float64).reshape(-1, 3) - p) @ R          # rows: R^T (X - p)
    with np.errstate(all="ignore"):
        uv = np.column_stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy])
    return uv, pc


def jacobians(prm, R, pc):
    """(n, 2, 6): de/dxi of every edge, xi = (dp, dtheta)"""
    n = len(pc)
    fx, fy, _, _ = intrinsics_of(prm)
    J = np.zeros((n, 2, 6))
    with np.errstate(all="ignore"):
        for i in range(n):
            x, y, z = pc[i]
            dpc = np.array([[fx / z, 0, -fx * x / (z * z)], [0, fy / z, -fy * y / (z * z)]])
            J[i, :, :3] = dpc @ (-R.T)
            J[i, :, 3:] = dpc @ skew(pc[i])
    return J


def reference(prm, q, p, X, obs):
    """dict: info, cov (None when degenerate by the definition's own test), chi2, sq_err, n_edges, n_inliers, n_borderline, status, e2 (per edge),
    near = edges within BORDER of the gate (their decision may go either way)"""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    obs = np.asarray(obs, np.float32).reshape(-1, 2).astype(np.float64)
    p = np.asarray(p, np.float64)
    R = quat_to_R(q)
    uv, pc = project(prm, R, p, X)
    with np.errstate(all="ignore"):
        e = uv - obs
        e2 = (e * e).sum(axis=1)
        inl = (pc[:, 2] > 0) & (e2 <= TH2)
        near = np.abs(e2 - TH2) < BORDER
    J = jacobians(prm, R, pc)
    info = np.zeros((6, 6))
    for i in np.flatnonzero(inl):
        info += (1.0 / (1.0 + e2[i] / TH2)) * (J[i].T @ J[i])
    out = {"info": info, "e2": e2, "inlier": inl, "near": near, "pc": pc, "J": J,
           "chi2": float((TH2 * np.log1p(e2[inl] / TH2)).sum()), "sq_err": float(e2[inl].sum()),
           "n_edges": len(X), "n_inliers": int(inl.sum()), "n_borderline": int(near.sum())}
    out["status"] = 1 if (out["n_inliers"] >= 3 and not degenerate(info)) else 2
    out["cov"] = np.linalg.inv(info) if out["status"] == 1 else None
    return out


def degenerate(info):
    """the definition's test: an LDL^T pivot d_k <= 1e-12 info[k][k] (no pivoting, natural order)"""
    A = np.array(info, np.float64)
    for k in range(6):
        d = A[k, k]
        if not (d > PIVOT_REL * info[k, k]) or not np.isfinite(d):
            return True
        l = A[k + 1:, k] / d
        A[k + 1:, k + 1:] -= np.outer(l, A[k + 1:, k])
    return False


def scaled(M, d):
    s = np.sqrt(np.outer(d, d))
    with np.errstate(all="ignore"):
        return np.where(s > 0, M / np.where(s > 0, s, 1.0), M)


def info_error(got, want):
    """max |dinfo_ij| / sqrt(info_ii info_jj)"""
    return float(np.abs(scaled(got - want, np.diag(want))).max())


def cov_errors(info_dev, cov_dev):
    """(max |info cov - I| with rows / columns scaled by sqrt(diag), max |dcov_ij| / sqrt(cov_ii cov_jj) against the inverse of the DEVICE's info)"""
    s = np.sqrt(np.diag(info_dev))
    ident = (info_dev / np.outer(s, s)) @ (cov_dev * np.outer(s, s))      # D^-1 info D^-1 . D cov D = D^-1 (info cov) D
    inv = np.linalg.inv(info_dev)
    return float(np.abs(ident - np.eye(6)).max()), float(np.abs(scaled(cov_dev - inv, np.diag(inv))).max())


def check_valid(rec, ref, what=""):
    """a status-1 record against the reference at the issue's bounds; returns the three observed figures"""
    info, cov = rec.info, rec.cov
    assert rec.status == 1 and ref["status"] == 1, (what, rec.status, ref["status"])
    assert np.array_equal(info, info.T) and np.array_equal(cov, cov.T), f"{what}: not exactly symmetric"
    e_info = info_error(info, ref["info"])
    e_ident, e_cov = cov_errors(info, cov)
    print(f"{what}: info {e_info:.2e} identity {e_ident:.2e} cov {e_cov:.2e} cond {np.linalg.cond(info):.2e}")
    assert e_info <= INFO_TOL, (what, e_info)
    assert e_ident <= IDENT_TOL, (what, e_ident)
    assert e_cov <= COV_TOL, (what, e_cov)
    return e_info, e_ident, e_cov


def check_counts(rec, ref, what=""):
    """counts and sums; exact where the reference finds no edge within BORDER of the gate"""
    assert rec.n_edges == ref["n_edges"], (what, rec.n_edges, ref["n_edges"])
    if not ref["near"].any():
        assert rec.n_inliers == ref["n_inliers"] and rec.n_borderline == 0, (what, rec.n_inliers, ref["n_inliers"], rec.n_borderline)
        for name in ("chi2", "sq_err"):
            got, want = getattr(rec, name), ref[name]
            assert abs(got - want) <= 1e-10 * max(abs(want), 1.0), (what, name, got, want)


def point_for(prm, R, p, obs, z, e2_target, direction):
    """A world point at camera depth z whose e.e against the float32 observation `obs` under (R, p) is e2_target, the error pointing along `direction`.
    A float32 observation near 10^3 px moves in steps of 6e-5 px (3e-4 in e.e at the gate), so the wanted value is reached through the point, which
    is float64: solve in the image, back-project, then CHECK with project().  Returns (X, the e.e project() finds)."""
    d = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    o = np.asarray(obs, np.float32).astype(np.float64)
    X = None
    scale = np.sqrt(e2_target)
    for _ in range(4):                 # (two rounds of correcting the length by what project() finds reach 1e-12)
        uv = o + scale * d
        fx, fy, cx, cy = intrinsics_of(prm)
        pc = np.array([(uv[0] - cx) * z / fx, (uv[1] - cy) * z / fy, z])
        X = R @ pc + p
        e = project(prm, R, p, X)[0][0] - o
        e2 = float(e @ e)
        if e2 > 0:
            scale *= np.sqrt(e2_target / e2)
    return X, e2
