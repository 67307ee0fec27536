"""The relocalisation search (include/lvt_amd_ext.h, RELOCALISATION) restated in numpy, stage by stage, for the tests.  Nothing here needs a GPU.

Arithmetic: the fp32 inputs are widened to fp64 and everything after that is fp64, one IEEE operation per written operation.  Sums and products are written
out element by element -- no matrix product, so neither a BLAS summation order nor an FMA enters -- and sums of three are ((a b + c d) + e f).  A comparison
that involves a NaN is false."""
import math

import numpy as np

NO_NEIGHBOUR = (-1, 0x7FFFFFFF)
ROW_RADIUS = 2
GOLDEN, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
MASK64 = (1 << 64) - 1
DEGENERATE = 1e-12
NF_MAX, MAP_MAX = 4096, 32768


# ---- stage 1: global match --------------------------------------------------------------------------------------------------------------------
def hamming_table(qd, td):
    """(N, M) integer Hamming distances of 256-bit descriptors: xor and popcount, 64 bits at a time"""
    q = np.ascontiguousarray(qd, np.uint8).reshape(-1, 32).view(np.uint64)
    t = np.ascontiguousarray(td, np.uint8).reshape(-1, 32).view(np.uint64)
    d = np.zeros((len(q), len(t)), np.int32)
    for w in range(4):
        d += np.bitwise_count(q[:, None, w] ^ t[None, :, w]).astype(np.int32)
    return d


def global_match(qd, td, chunk=256):
    """(N, 4) int32 records (idx1, d1, idx2, d2): every query's two nearest of ALL train descriptors, ties to the lowest index; NO_NEIGHBOUR where
    there is none -- the contract of pyoracle.hamming_top2(query, train)"""
    N, M = len(qd), len(td)
    out = np.empty((N, 4), np.int32)
    out[:, 0::2], out[:, 1::2] = NO_NEIGHBOUR
    if N == 0 or M == 0:
        return out
    assert M <= 65536
    idx = np.arange(M, dtype=np.int32)[None, :]
    for s in range(0, N, chunk):
        key = hamming_table(qd[s:s + chunk], td) * np.int32(65536) + idx       # distinct keys: the minimum is the (distance, index) order's
        rows = np.arange(len(key))
        for k in range(min(2, M)):
            j = np.argmin(key, axis=1)
            kk = key[rows, j]
            out[s:s + chunk, 2 * k] = kk & 0xFFFF
            out[s:s + chunk, 2 * k + 1] = kk >> 16
            key[rows, j] = np.int32(1 << 30)
    return out


def accept_match(cnt, d1, d2, ratio, desc_th):
    """the tracker's own rule (k_track.hip accept_match): two candidates -- d1 / d2 < ratio in fp32, so 0 / 0 fails; one -- d1 <= desc_th"""
    if cnt > 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            return bool(np.float32(d1) / np.float32(d2) < np.float32(ratio))
    if cnt == 1:
        return bool(np.float32(d1) <= np.float32(desc_th))
    return False


# ---- stage 2: correspondences -------------------------------------------------------------------------------------------------------------------
def correspondences(records, n_map, ratio, desc_th):
    """(feature index, map index) arrays, ordered by feature index, and n_matched.  A map point claimed by several features keeps the one with the
    smallest (d1, i)."""
    cnt = min(n_map, 2)
    claim = {}
    n_matched = 0
    for i, (i1, d1, i2, d2) in enumerate(np.asarray(records).tolist()):
        if not accept_match(cnt, d1, d2, ratio, desc_th):
            continue
        n_matched += 1
        if i1 not in claim or (d1, i) < claim[i1]:
            claim[i1] = (d1, i)
    pairs = sorted((i, m) for m, (_, i) in claim.items())[:NF_MAX]
    feat = np.array([p[0] for p in pairs], np.int64)
    mp = np.array([p[1] for p in pairs], np.int64)
    return feat, mp, n_matched


def back_project(x, y, Z, prm):
    """Pc = ((x - cx) Z / fx, (y - cy) Z / fy, Z), fp64 on the widened fp32 inputs"""
    fx, fy, cx, cy = (float(np.float32(v)) for v in (prm.fx, prm.fy, prm.cx, prm.cy))
    x, y, Z = float(x), float(y), float(Z)
    return (((x - cx) * Z) / fx, ((y - cy) * Z) / fy, Z)


def camera_points_rgbd(feat, xy, depth, prm):
    """every correspondence has a point: the depth the feature gather kept"""
    pc = np.zeros((len(feat), 3))
    for c, i in enumerate(feat):
        pc[c] = back_project(xy[i, 0], xy[i, 1], depth[i], prm)
    return pc, np.ones(len(feat), bool)


def camera_points_stereo(feat, xy_l, desc_l, xy_r, desc_r, prm, min_disparity, rows):
    """the stereo partner of each correspondence's left feature: row band (make_query_row: (float)max((int)y - 2, 0) <= y_r <= (float)min((int)y + 2, H)),
    x_l - x_r >= min_disparity in fp32, top two by Hamming distance (ties to the lowest j), the tracker's accept rule with the triangulation ratio.
    No exclusivity between left features."""
    pc = np.zeros((len(feat), 3))
    has = np.zeros(len(feat), bool)
    if len(xy_r) == 0:
        return pc, has
    xr, yr = xy_r[:, 0].astype(np.float32), xy_r[:, 1].astype(np.float32)
    fxb = float(np.float32(prm.fx)) * float(np.float32(prm.baseline))
    for c, i in enumerate(feat):
        xl, yl = np.float32(xy_l[i, 0]), np.float32(xy_l[i, 1])
        lo, hi = np.float32(max(int(yl) - ROW_RADIUS, 0)), np.float32(min(int(yl) + ROW_RADIUS, rows))
        cand = np.flatnonzero((yr >= lo) & (yr <= hi) & ((xl - xr).astype(np.float32) >= np.float32(min_disparity)))
        if len(cand) == 0:
            continue
        d = hamming_table(desc_l[i:i + 1], desc_r[cand])[0].astype(np.int64)
        key = np.sort(d * 65536 + cand)
        d1, j = int(key[0] >> 16), int(key[0] & 0xFFFF)
        d2 = int(key[1] >> 16) if len(key) > 1 else 0
        if not accept_match(min(len(cand), 2), d1, d2, prm.triangulation_ratio_test_threshold, prm.descriptor_matching_threshold):
            continue
        Z = fxb / (float(xl) - float(xr[j]))
        pc[c] = back_project(xl, yl, Z, prm)
        has[c] = True
    return pc, has


# ---- stage 3: hypotheses ------------------------------------------------------------------------------------------------------------------------
def sample(seed, h, j, n3):
    """number of the sampled correspondence among those with a point: splitmix64 of seed + (3 h + j + 1) golden"""
    x = (int(seed) + (3 * h + j + 1) * GOLDEN) & MASK64
    x ^= x >> 30
    x = (x * MIX1) & MASK64
    x ^= x >> 27
    x = (x * MIX2) & MASK64
    x ^= x >> 31
    return x % n3


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def triad(p0, p1, p2):
    """(e1, e2, e3) of three points as Python floats, or None when degenerate"""
    p0, p1, p2 = ([float(v) for v in p] for p in (p0, p1, p2))
    d = [p1[k] - p0[k] for k in range(3)]
    n1 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    if n1 <= DEGENERATE:
        return None
    l1 = math.sqrt(n1)      # (a NaN passes through, as everywhere below: the hypothesis then has no inlier)
    e1 = [v / l1 for v in d]
    b = [p2[k] - p0[k] for k in range(3)]
    c = cross(e1, b)
    n3 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
    if n3 <= DEGENERATE:
        return None
    l3 = math.sqrt(n3)
    e3 = [v / l3 for v in c]
    e2 = list(cross(e3, e1))
    return e1, e2, e3


def hypothesis(seed, h, with_pc, pc, X):
    """(R (3, 3) camera to world, t (3,)) of hypothesis h, or None when it scores 0 (coincident samples, a degenerate triad)"""
    n3 = len(with_pc)
    s = [sample(seed, h, j, n3) for j in range(3)]
    if s[0] == s[1] or s[0] == s[2] or s[1] == s[2]:
        return None
    idx = [int(with_pc[k]) for k in s]
    a = [[float(v) for v in pc[i]] for i in idx]
    b = [[float(v) for v in X[i]] for i in idx]
    with np.errstate(all="ignore"):
        Ea, Eb = triad(*a), triad(*b)
    if Ea is None or Eb is None:
        return None
    ma = [((a[0][k] + a[1][k]) + a[2][k]) / 3.0 for k in range(3)]
    mb = [((b[0][k] + b[1][k]) + b[2][k]) / 3.0 for k in range(3)]
    R = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            R[i, j] = (Eb[0][i] * Ea[0][j] + Eb[1][i] * Ea[1][j]) + Eb[2][i] * Ea[2][j]
    t = np.zeros(3)
    for i in range(3):
        t[i] = mb[i] - ((R[i, 0] * ma[0] + R[i, 1] * ma[1]) + R[i, 2] * ma[2])
    return R, t


# ---- stage 4: score -----------------------------------------------------------------------------------------------------------------------------
def inlier_mask(R, t, X, uv, prm, gate_px2):
    """(n,) bool over EVERY correspondence: pcz > 0 and e.e <= gate_px2, false for NaN"""
    fx, fy, cx, cy = (float(np.float32(v)) for v in (prm.fx, prm.fy, prm.cx, prm.cy))
    X = np.asarray(X, np.float64).reshape(-1, 3)
    u, v = np.asarray(uv, np.float32).reshape(-1, 2).astype(np.float64).T
    with np.errstate(all="ignore"):
        dx, dy, dz = X[:, 0] - t[0], X[:, 1] - t[1], X[:, 2] - t[2]
        px = (R[0, 0] * dx + R[1, 0] * dy) + R[2, 0] * dz
        py = (R[0, 1] * dx + R[1, 1] * dy) + R[2, 1] * dz
        pz = (R[0, 2] * dx + R[1, 2] * dy) + R[2, 2] * dz
        ex = ((fx * px) / pz + cx) - u
        ey = ((fy * py) / pz + cy) - v
        return (pz > 0.0) & ((ex * ex + ey * ey) <= float(np.float32(gate_px2)))


def score_all(seed, n_hyp, with_pc, pc, X, uv, prm, gate_px2):
    """counts (n_hyp,) int32 and the hypotheses themselves (None where one scores 0)"""
    counts = np.zeros(n_hyp, np.int32)
    hyps = [None] * n_hyp
    if len(with_pc) < 3:
        return counts, hyps
    for h in range(n_hyp):
        hyps[h] = hypothesis(seed, h, with_pc, pc, X)
        if hyps[h] is not None:
            counts[h] = int(inlier_mask(hyps[h][0], hyps[h][1], X, uv, prm, gate_px2).sum())
    return counts, hyps


# ---- stage 5: refine ----------------------------------------------------------------------------------------------------------------------------
def mat3_to_quat(R):
    """rotation matrix -> quaternion (w, x, y, z): the branch on the trace / largest diagonal element (lvt_odometry.h mat3_to_quat)"""
    R = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
    q = [0.0] * 4
    tr = R[0] + R[4] + R[8]
    if tr > 0:
        s = math.sqrt(tr + 1.0)
        r = 0.5 / s
        q[0] = 0.5 * s
        q[1], q[2], q[3] = (R[7] - R[5]) * r, (R[2] - R[6]) * r, (R[3] - R[1]) * r
    else:
        i = 0
        if R[4] > R[0]:
            i = 1
        if R[8] > R[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        s = math.sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0)
        r = 0.5 / s
        q[1 + i] = 0.5 * s
        q[0] = (R[3 * k + j] - R[3 * j + k]) * r
        q[1 + j] = (R[3 * j + i] + R[3 * i + j]) * r
        q[1 + k] = (R[3 * k + i] + R[3 * i + k]) * r
    return np.array(q)


def success_count(cfg, prm):
    return max(int(cfg["min_inliers"]), int(prm.min_num_matches_for_tracking))


DEFAULTS = dict(n_hypotheses=256, gate_px2=16.0, min_disparity=1.0, min_inliers=30, seed=0, dry_run=0)


def solve(prm, X, uv, pc, has_pc, cfg=None, pnp=None):
    """stages 3 - 5 on given correspondences.  `pnp(prm, q0, p0, pts, obs) -> (q, p, inlier marks)` is the refinement (pyoracle.pnp's first three
    results); without one the call stops behind stage 4 with status None.  Returns a dict with the result record's fields, counts, inliers, hyp_R, hyp_t,
    start_q."""
    cfg = dict(DEFAULTS, **(cfg or {}))
    X = np.asarray(X, np.float64).reshape(-1, 3); uv = np.asarray(uv, np.float32).reshape(-1, 2); pc = np.asarray(pc, np.float64).reshape(-1, 3)
    with_pc = np.flatnonzero(np.asarray(has_pc).astype(bool))
    n_hyp = int(cfg["n_hypotheses"])
    out = dict(status=1, n_corr=len(X), n_with_point=len(with_pc), best_hypothesis=0, n_hyp_inliers=0, n_refined_inliers=0,
               q=np.zeros(4), p=np.zeros(3), counts=np.zeros(n_hyp, np.int32), inliers=np.zeros(0, np.int64), hyp_R=np.zeros((3, 3)), hyp_t=np.zeros(3))
    if len(with_pc) < 3:
        return out
    counts, hyps = score_all(cfg["seed"], n_hyp, with_pc, pc, X, uv, prm, cfg["gate_px2"])
    best = int(np.argmax(counts))                      # (the first of equal counts: ties to the lowest h)
    out.update(counts=counts, best_hypothesis=best, n_hyp_inliers=int(counts[best]), status=2)
    need = success_count(cfg, prm)
    if counts[best] < need:
        return out
    R, t = hyps[best]
    inl = np.flatnonzero(inlier_mask(R, t, X, uv, prm, cfg["gate_px2"]))
    q0 = mat3_to_quat(R)
    out.update(inliers=inl, hyp_R=R, hyp_t=t, start_q=q0, status=None)
    if pnp is None:
        return out
    q, p, marks = pnp(prm, q0, t, X[inl], uv[inl])[:3]
    n_ref = int(np.asarray(marks).sum())
    finite = bool(np.isfinite(q).all() and np.isfinite(p).all())
    out.update(q=np.asarray(q), p=np.asarray(p), n_refined_inliers=n_ref, status=0 if (finite and n_ref >= need) else 3)
    return out


# ---- stage 6: what a commit leaves ----------------------------------------------------------------------------------------------------------------
def committed_state(q, p, n_refined):
    """the tracker state behind a successful, committed call: TRACKING at the refined pose, the motion model at rest there"""
    return dict(state=2, last_pose=(np.asarray(q), np.asarray(p)), mm_last_q=np.asarray(q), mm_last_p=np.asarray(p), mm_ang_vel=np.array([1.0, 0, 0, 0]),
                mm_lin_vel=np.zeros(3), mm_pending=0, last_matches=(n_refined,) * 3, early_done=0, early_accepted=0)


# ---- the whole search ---------------------------------------------------------------------------------------------------------------------------
def relocalise(prm, sensor, map_xyz, map_desc, xy_l, desc_l, right=None, depth=None, cfg=None, pnp=None):
    """stages 1 - 5 on a map and one frame's features.  right = (xy_r, desc_r) for stereo, depth = (N,) float32 for RGB-D"""
    cfg = dict(DEFAULTS, **(cfg or {}))
    M = min(len(map_xyz), MAP_MAX)
    rec = global_match(desc_l, map_desc[:M])
    feat, mp, n_matched = correspondences(rec, M, prm.tracking_ratio_test_threshold, prm.descriptor_matching_threshold)
    if sensor == 2:
        pc, has = camera_points_rgbd(feat, xy_l, depth, prm)
    else:
        pc, has = camera_points_stereo(feat, xy_l, desc_l, right[0], right[1], prm, cfg["min_disparity"], prm.img_height)
    out = solve(prm, np.asarray(map_xyz)[mp], np.asarray(xy_l, np.float32)[feat], pc, has, cfg, pnp)
    out.update(n_features=len(xy_l), n_map=M, n_matched=n_matched, feat=feat, map_idx=mp, pc=pc, has_pc=has, records=rec)
    return out
