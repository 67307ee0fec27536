"""The inputs of the edge-case tests of k_pnp and k_triangulate, in one place: the GPU tests (test_gpu_primitives.py, test_gpu_parity.py,
test_gpu_mixed_batch.py) drive the HIP path with them, the CPU tier (test_case_tables.py) asserts with the oracle alone that they still take
the branches they were chosen for.  Nothing here needs a GPU."""
import numpy as np

import lvt_amd

# k_pnp's constants (k_track.hip): a wavefront, PNP_THREADS, PNP_ILP * PNP_THREADS (one sweep iteration), PNP_STAGE_MAX (above it the edges stay
# in global memory), NF_MAX -- each with its neighbours -- and the counts below 8 (H has rank < 6 for n <= 2: the solve leans on the damping)
PNP_EDGE_COUNTS = [0, 1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1535, 1536, 1537, 2047, 2048, 2049, 3000,
                   4095, 4096]
PNP_INTRINSICS = ("kitti", "tum", "euroc")      # TUM: fx != fy
PNP_STAGE_MAX = 1536


def intrinsics(name):
    return {"kitti": lvt_amd.kitti_params, "tum": lvt_amd.tum_params, "euroc": lvt_amd.euroc_params}[name]()


def pnp_case(rng, prm, n):
    """n points in front of a camera ~0.3 m / ~0.6 degrees off the identity prior, observations rounded to pixels, every ninth a 25-px outlier"""
    X = np.column_stack([rng.uniform(-20, 20, n), rng.uniform(-5, 5, n), rng.uniform(6, 60, n)])
    ang = rng.normal(0, 0.01, 3)
    q = np.array([1.0, *(ang / 2)]); q /= np.linalg.norm(q)
    p_true = rng.normal(0, 0.3, 3)
    w, x, y, z = q
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    Xc = (X - p_true) @ Rm
    uv = np.column_stack([prm.fx * Xc[:, 0] / Xc[:, 2] + prm.cx, prm.fy * Xc[:, 1] / Xc[:, 2] + prm.cy])
    uv = np.rint(uv + rng.normal(0, 0.4, uv.shape)).astype(np.float32)
    uv[::9] += 25.0
    return X, uv


def pnp_edge_case(name, n):
    """(params, X, uv, q0, p0) of one edge-count case: seeded by n alone, identity prior"""
    prm = intrinsics(name)
    X, uv = pnp_case(np.random.default_rng(1000 + n), prm, n)
    return prm, X, uv, np.array([1.0, 0, 0, 0]), np.zeros(3)


def pnp_hard_case(prm, seed, n, off_t, off_deg, outl, big):
    """prior `off_t` metres / `off_deg` degrees away from the truth (identity), a fraction `outl` of gross outliers up to `big` pixels"""
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(-20, 20, n), rng.uniform(-5, 5, n), rng.uniform(6, 60, n)])
    uv = np.column_stack([prm.fx * X[:, 0] / X[:, 2] + prm.cx, prm.fy * X[:, 1] / X[:, 2] + prm.cy])
    uv = np.rint(uv + rng.normal(0, 0.4, uv.shape)).astype(np.float32)
    k = rng.random(n) < outl
    uv[k] += rng.uniform(-big, big, (int(k.sum()), 2)).astype(np.float32)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    a = np.deg2rad(off_deg)
    q0 = np.array([np.cos(a / 2), *(np.sin(a / 2) * ax)])
    d = rng.normal(size=3); d /= np.linalg.norm(d)
    return X, uv, q0, off_t * d


# (seed, n, metres off, degrees off, outlier fraction, outlier size): chosen by running the ORACLE over seeds (tests/tools/pnp_hard_cases.py) so that the
# branches of A.6 a good prior never reaches are taken: rejected trials, Terminate, and a step with |delta| > 1 whose sqrt(1 - |delta|^2) is NaN
PNP_HARD = [(25, 200, 2.0, 15, 0.3, 200), (12, 60, 5, 60, 0.5, 400), (24, 60, 5, 60, 0.5, 400), (2, 40, 8, 120, 0.5, 400), (11, 40, 8, 120, 0.5, 400),
            (4, 30, 10, 170, 0.3, 100), (30, 30, 10, 170, 0.3, 100), (31, 30, 10, 170, 0.3, 100), (7, 300, 1.5, 10, 0.3, 25)]
# the same search at n = 1600, 2500, 4096 (python tests/tools/pnp_hard_cases.py 1600 2500 4096): above PNP_STAGE_MAX the edges, their errors and
# the inactive lanes' sink stay in global memory, and pop() leaves a rejected trial's errors there in front of the 5.991 gate
PNP_HARD_UNSTAGED = [
    # comparable to their last trial: 1, 1, 3 rejections; 1 rejection + NaN step; 1; 7 + NaN step; 3; 2; 2
    (2, 1600, 10, 170, 0.3, 100), (8, 1600, 10, 170, 0.3, 100), (33, 1600, 10, 170, 0.3, 100), (23, 2500, 8, 120, 0.5, 400),
    (0, 2500, 10, 170, 0.3, 100), (11, 2500, 10, 170, 0.3, 100), (39, 2500, 10, 170, 0.3, 100), (39, 4096, 8, 120, 0.5, 400),
    (2, 4096, 10, 170, 0.3, 100),
    # with a Terminate (a noise-level trial ends the trial-by-trial comparison early); the last one: 4 rejections, 1 Terminate
    (6, 1600, 5, 60, 0.5, 400), (20, 2500, 5, 60, 0.5, 400), (30, 4096, 5, 60, 0.5, 400), (28, 4096, 10, 170, 0.3, 100)]


def trace_noise(tr):
    """index of the first trial whose chi2 equals the estimate's to ~10 digits (its accept / reject decision is taken on the last bits of two sums
    over all edges: no two summation orders agree on it), len(tr) without one"""
    d = np.abs(tr[:, 1] - tr[:, 2]) <= 1e-10 * np.abs(tr[:, 1])
    return int(np.argmax(d)) if d.any() else len(tr)


def pnp_prior_cases(prm):
    """A.6's SE3Quat constructor normalises the prior and flips it to w >= 0: the same rotation given as q, -q, 3 q and an unnormalised quaternion
    with w < 0 must lead to one solve.  n = 40 / 300 / 1700 with 10 % of the points mirrored behind the camera (g2o has no cheirality test:
    their edges are ordinary gross outliers with pcz < 0), and one case whose outliers are graded 10^k px, k = 0 .. 5 (log_ge1 over its argument
    range).  Yields (label, X, uv, [priors], p0)."""
    for n in (40, 300, 1700):
        rng = np.random.default_rng(2000 + n)
        X, uv = pnp_case(rng, prm, n)
        k = rng.random(n) < 0.1
        X[k, 2] = -X[k, 2]
        raw = np.array([-0.5, 0.001, -0.002, 0.0015])
        q = -raw / np.linalg.norm(raw)
        yield f"behind_{n}", X, uv, [q, -q, 3 * q, raw], np.zeros(3)
    rng = np.random.default_rng(2999)
    X, uv = pnp_case(rng, prm, 600)
    for j in range(0, 600, 9):
        uv[j] += np.float32(10.0 ** ((j // 9) % 6) - 25.0)      # (pnp_case put 25 px there)
    yield "graded_outliers", X, uv, [np.array([1.0, 0, 0, 0])], np.zeros(3)


# ---- the pipeline above the staging limit -----------------------------------------------------------------------------------------------------
# name, kind, seed, scale, overrides, frame ids: ~2 400 features per image and triangulation on every frame; from frame 2 on more than PNP_STAGE_MAX matches
KITTI_DENSE_UNSTAGED = ("kitti_dense_unstaged", "kitti", 2, 1.0,
                        {"agast_threshold": 6, "max_keypoints_per_cell": 1000, "triangulation_policy": 2, "staged_threshold": 0}, list(range(10)))
DENSE_MIN_UNSTAGED_FRAMES = 6


# ---- triangulation gates: a planted disparity staircase -----------------------------------------------------------------------------------------
STAIR_W, STAIR_BAND = 1241, 94
STAIR_NEAR, STAIR_FAR = 2.0, 40.0
# (disparity, rows the right eye's band is moved down): behind the camera, parallel rays, far beyond far, beyond far on both sides of 9.6536 px, inside,
# nearer than near on both sides of 193.07 px
STAIRCASE = {
    "13_bands": [(d, 0) for d in (-5, 0, 0.4, 5, 9.4, 9.6, 9.7, 12, 40, 150, 192.9, 193.3, 300)],          # H = 1222: row lists past LS_BINS
    "11_bands": [(d, 0) for d in (-5, 0, 0.4, 9.4, 9.6, 9.7, 12, 150, 192.9, 193.3, 300)],                  # H = 1034: the binned kernel builds them
    "row_band_edge": [(12, 0), (12, 2), (12, 3), (150, 0)],                                                  # the edge of row_match's +-2 row band
}
STAIR_ROWS = (40, 47, 54)


def staircase(variant):
    """one stereo frame of noise cut into bands of 94 rows; the right eye's band b is the left one moved d_b px to the left (and dy_b rows down), with
    external corners on three rows of every band: left (x, y), right (x - d_b, y + dy_b).  BRIEF rounds a fractional corner to its pixel, so the
    descriptors of a pair are identical and every corner pairs with its own partner -- what is decided per band is the triangulation alone.
    Returns (params, L, R, corners_left, corners_right, bands)."""
    bands = STAIRCASE[variant]
    W, H = STAIR_W, STAIR_BAND * len(bands)
    prm = lvt_amd.kitti_params(width=W, height=H)
    prm.far_plane_distance, prm.near_plane_distance = STAIR_FAR, STAIR_NEAR
    rng = np.random.default_rng(0)
    L = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    R = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    xs = np.arange(340, W - 40, 23, dtype=np.float64)
    cl, cr = [], []
    for b, (d, dy) in enumerate(bands):
        y0 = b * STAIR_BAND
        band = np.roll(L[y0:y0 + STAIR_BAND], -int(np.floor(d + 0.5)), axis=1)
        R[y0:y0 + STAIR_BAND] = np.roll(band, dy, axis=0)
        for r in STAIR_ROWS:
            cl.append(np.column_stack([xs, np.full_like(xs, y0 + r)]))
            cr.append(np.column_stack([xs - d, np.full_like(xs, y0 + r + dy)]))
    return prm, L, np.ascontiguousarray(R), np.vstack(cl), np.vstack(cr), bands


def staircase_expected(prm, bands):
    """per band: (pairs, map points) predicted from z = fx b / d against the two planes; a band moved down more than 2 rows does not pair"""
    per_band = len(STAIR_ROWS) * len(np.arange(340, STAIR_W - 40, 23))
    out = []
    for d, dy in bands:
        pairs = per_band if abs(dy) <= 2 else 0
        z = prm.fx * prm.baseline / d if d > 0 else -1.0
        # (the nearest band, 192.9 px at z = 2.0018, sits 8.9e-4 relative from its plane: nine orders of magnitude above the fp64 error of the solve)
        assert d <= 0 or min(abs(z / STAIR_NEAR - 1), abs(z / STAIR_FAR - 1)) > 5e-4
        out.append((pairs, pairs if STAIR_NEAR <= z <= STAIR_FAR else 0))
    return out


def staircase_band_counts(prm, xyz, n_bands):
    """map points per band, a point's band taken from its row in the (identity-pose) left image"""
    v = prm.fy * xyz[:, 1] / xyz[:, 2] + prm.cy
    return np.bincount(np.floor(v / STAIR_BAND).astype(np.int64), minlength=n_bands)[:n_bands].tolist() if len(xyz) else [0] * n_bands


# ---- the map kernels from 10k points to past capacity ----------------------------------------------------------------------------------------------
# Four recipes that take the per-frame map kernels (bookkeep_cull_large, the super-chunk resolver, staged_body, the two capacity cuts) to the sizes
# they are written for: MAP_MAX map points, several thousand staged points.  Every frame is noise; columns [0, 300) are the same in all frames (the
# pose stays solvable on the corners there), the rest is fresh per texture epoch, so old map points find no partner and every fresh corner
# triangulates.  The right eye is the left one moved 12 px (z ~ 32 m).
MAP_MAX, STAGED_MAX = 32768, 16384        # lvt_dev.h
MAPCAP_W, MAPCAP_H, MAPCAP_DISP = 1241, 376, 12
MAPCAP_KEEP, MAPCAP_FRESH = 300, 3700

# name: (overrides, frames per texture epoch, external corners, frames).  `steady` culls as fast as it appends and plateaus below MAP_MAX; `direct`
# appends past MAP_MAX by triangulation, `promotion` by promotion of staged points (staged on even frames, promoted on odd ones); `detector` is
# `direct` through the detector (plain track): the lock-step batch's case; `direct_recover` overflows, then culls its way back below the capacity
MAPCAP_RECIPES = {
    "steady": ({"staged_threshold": 0, "untracked_threshold": 8}, 1, True, 14),
    "direct": ({"staged_threshold": 0, "untracked_threshold": 1000}, 1, True, 12),
    "direct_recover": ({"staged_threshold": 0, "untracked_threshold": 10}, 1, True, 14),
    "promotion": ({"staged_threshold": 1, "untracked_threshold": 1000}, 2, True, 22),
    "detector": ({"staged_threshold": 0, "untracked_threshold": 1000, "max_keypoints_per_cell": 400}, 1, False, 18),
}


def mapcap_params(name):
    prm = lvt_amd.kitti_params(width=MAPCAP_W, height=MAPCAP_H)
    prm.triangulation_policy = 2
    for k, v in MAPCAP_RECIPES[name][0].items():
        setattr(prm, k, type(getattr(prm, k))(v))
    return prm


def _mapcap_fixed():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (MAPCAP_H, MAPCAP_W), dtype=np.uint8)
    keep = np.column_stack([rng.integers(52, 270, MAPCAP_KEEP), rng.integers(40, MAPCAP_H - 40, MAPCAP_KEEP)])
    return img, keep


def mapcap_frame(epoch):
    """(L, R, corners_left, corners_right) of one texture epoch"""
    fixed, keep = _mapcap_fixed()
    rng = np.random.default_rng(100 + epoch)
    L = rng.integers(0, 256, (MAPCAP_H, MAPCAP_W), dtype=np.uint8)
    L[:, :300] = fixed[:, :300]
    R = np.ascontiguousarray(np.roll(L, -MAPCAP_DISP, axis=1))
    fresh = np.column_stack([rng.integers(340, MAPCAP_W - 40, MAPCAP_FRESH), rng.integers(40, MAPCAP_H - 40, MAPCAP_FRESH)])
    cl = np.unique(np.vstack([keep, fresh]), axis=0).astype(np.float64)
    return L, R, cl, cl - [[float(MAPCAP_DISP), 0.0]]


def mapcap_case(name, n_frames=None):
    """(params, generator of (L, R, corners_left, corners_right)); the corner lists are None for a recipe that runs through the detector.  Frames are
    made one at a time: a stereo pair is 0.9 MB"""
    _, per_epoch, ext, n = MAPCAP_RECIPES[name]

    def frames():
        for i in range(n_frames or n):
            L, R, cl, cr = mapcap_frame(i // per_epoch)
            yield (L, R, cl, cr) if ext else (L, R, None, None)
    return mapcap_params(name), frames()


def mapcap_track(system, frame):
    """one recipe frame through an oracle or a HIP handle (the two share the method names)"""
    L, R, cl, cr = frame
    return system.track(L, R) if cl is None else system.track_with_external_corners(L, R, cl, cr)
