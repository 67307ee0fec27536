"""The inputs of the edge-case tests of k_pnp and k_triangulate, in one place: the GPU tests (test_gpu_primitives.py, test_gpu_parity.py,
test_gpu_mixed_batch.py) drive the HIP path with them, the CPU tier (test_case_tables.py) asserts with the oracle alone that they still take
the branches they were chosen for.  Further down: the planted scenes of the triangulation gates, the map capacity, the resolver chains and the RGB-D
depth and lens edges (test_gpu_rgbd_edges.py), held the same way.  Nothing here needs a GPU."""
import functools

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


# ---- the greedy match resolvers on deep dependency chains: the "domino" scenes ---------------------------------------------------------------------
# The resolvers (resolve_super and its callers, k_track.hip) replace the reference's serial accept / mark scans by a synchronous fixpoint that needs
# one iteration more than the longest chain "query q's best candidate is taken by an earlier query" is long.  Random texture gives chains of 2 - 4.
# A domino scene builds one of any length out of image content alone: BRIEF reads 9 x 9 box sums at offsets <= 24, so the descriptor of a corner is
# a function of its own 57 x 57 patch.
#   nodes      integer positions on a lattice of pitch 58, numbered boustrophedon: consecutive nodes are lattice neighbours
#   frame 0    left eye: node i carries its own noise patch P_i.  Right eye: node j, moved DOMINO_DISP px to the left, carries the blend
#              a P_(j+1) + (1 - a) P_j: its descriptor is nearest to desc(P_(j+1)), second nearest to desc(P_j), far from every other patch
#   frame >= 1 left eye: the blends at the nodes' own positions (static camera); right eye: the same image moved DOMINO_DISP px
# row_match (frame 0) and find_matches (frame >= 1, tracking radius 60: a map point sees its four lattice neighbours and itself) then meet the same
# preference: query i takes target i - 1 before target i before anything else.  Serially query 0 takes target 0 (target -1 does not exist) and every
# later query is pushed to its own target; in the fixpoint query i cannot settle before iteration i + 1.  row_match offers a query the targets of
# its own lattice row only (+-2 rows, any x), so there every lattice row is a chain of its own, all running at once.
# Fillers are plain corners on the scene's noise background, identical in every frame and eye: each matches itself at distance 0.
#
# Noise patches drawn blindly spread too far for a chain of a hundred (at a = 0.6 best 26 .. 60, second 54 .. 114, unrelated pairs down to 82 were
# measured: some node always breaks the chain), so the patches are drawn until they meet fixed windows (domino_patches).  Measured with the oracle's
# BRIEF on `map_chain` (test_case_tables.py asserts these figures), per chain query behind the head (best, second, third) as min / median / max:
#   find_matches, frames 1 and 2   best 36 / 47 / 54     second 70 / 77 / 86     third 101 / 117 / 152
#   row_match, frame 0             best 36 / 47 / 54     second 70 / 77 / 86     third 100 / 108 / 118
# so best / second <= 0.78 and second / third <= 0.86 at the worst node.  Both ratio thresholds are set to 0.9: the chain conditions hold with room
# (at the reference's defaults, 0.8 and 0.6, a query pushed off its best candidate would be left unmatched and its successor let through).
# Measured depths (synchronous fixpoint on the oracle's own candidate lists, counting the last iteration, which changes nothing):
#   map_chain                    96 (95 queries in one chain)          row_chain   20 (five chains of 19, one per lattice row)
#   chain_across_super_chunks    super-chunk 0: 48, super-chunk 1: 49  staged_chain 96 (update_staged's scan over the 95 staged chain points)
DOMINO_PITCH, DOMINO_HALF, DOMINO_DISP, DOMINO_RADIUS, DOMINO_ALPHA, DOMINO_RATIO = 58, 28, 20, 60, 0.6, 0.9
DOMINO_BEST, DOMINO_SECOND, DOMINO_OTHER = (36, 54), (70, 86), 100      # Hamming distances the chain's patches are drawn for (domino_patches)
RES_QCAP, RES_LCAP, RES_KC, RES_THREADS = 2048, 24576, 128, 1024        # k_track.hip / lvt_dev.h: queries and packed list entries of a super-chunk


def boustrophedon(cols, rows, x0, y0, pitch=DOMINO_PITCH):
    """integer lattice positions, row by row, every second row from right to left"""
    out = []
    for r in range(rows):
        cs = range(cols) if r % 2 == 0 else range(cols - 1, -1, -1)
        out += [(x0 + pitch * c, y0 + pitch * r) for c in cs]
    return np.array(out, dtype=np.int64)


# name: (width, height, lattice (cols, rows, x0, y0), dense fillers (cols, rows, x0, y0, pitch) or None, sparse fillers (cols, x0, y0, pitch) or None,
#        staged_threshold, frames)
DOMINO_SCENES = {
    "map_chain": (1241, 376, (19, 5, 70, 60), None, None, 0, 3),
    "chain_across_super_chunks": (2048, 1040, (19, 5, 70, 60), (48, 16, 60, 400, 16), (39, 930, 400, 28), 0, 3),
    # the same scene and corner order, staged_threshold 1.  Frame 0 is given the fillers alone: they are the 250 map points without which every staged
    # point is promoted at once.  Frame 1 adds the chain's corners on frame 0's images: the fillers match the map, the chain's pairs are staged (in
    # corner order: the whole chain, then the spares).  Frame 2 shows the blends: the chain runs through update_staged's resolver and is promoted; the
    # spares of the first three lattice rows are left out of its corners, so their staged points are erased
    "staged_chain": (2048, 1040, (19, 5, 70, 60), (48, 16, 60, 400, 16), (39, 930, 400, 28), 1, 3),
}
STAGED_CHAIN_DROPPED = 3
DOMINO_MIN_DEPTH = {"map_chain": 64, "row_chain": 16, "chain_across_super_chunks": 32}


def super_chunks(n_cand):
    """the resolver's cut of a query list into super-chunks (resolve_super): at most QCAP queries, the longest prefix whose lists (lengths rounded
    up to 4 entries) fit LCAP packed entries; a query with more than KC candidates ends the chunk in front of it and is decided alone (length 1)"""
    out, b0, M = [], 0, len(n_cand)
    while b0 < M:
        if n_cand[b0] > RES_KC:
            out.append((b0, 1)); b0 += 1
            continue
        used, ent = 0, 0
        while b0 + used < M and used < RES_QCAP and n_cand[b0 + used] <= RES_KC and ent + ((n_cand[b0 + used] + 3) & ~3) <= RES_LCAP:
            ent += (n_cand[b0 + used] + 3) & ~3
            used += 1
        out.append((b0, used)); b0 += used
    return out


def _neighbour_counts(xy, radius):
    d2 = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)
    return (d2 < radius * radius).sum(1)


def _blend(a, b):
    return np.rint(DOMINO_ALPHA * a.astype(np.float64) + (1.0 - DOMINO_ALPHA) * b.astype(np.float64)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def domino_patches(n, n_spare):
    """(P, blend, spare): n + 1 noise patches of 57 x 57, the n blends a P_(i+1) + (1 - a) P_i, and n_spare patches for the spare corners.  P_(i+1) is
    drawn, seeded, until blend_i lies within DOMINO_BEST of desc(P_(i+1)) and within DOMINO_SECOND of desc(P_i), and every unrelated pair (a blend, a
    patch) of the chain so far is at least DOMINO_OTHER apart; a spare is at least DOMINO_OTHER from every patch and blend.  The descriptor of a patch
    is the oracle's BRIEF at its centre (it reads nothing outside the patch)."""
    from oracle import pyoracle as O
    side, batch = 2 * DOMINO_HALF + 1, 32
    centres = np.array([[DOMINO_HALF + side * k, DOMINO_HALF] for k in range(batch)], dtype=np.float32)

    def desc(patches):
        kept, d = O.brief(np.ascontiguousarray(np.hstack(list(patches))), centres[:len(patches)])
        assert len(kept) == len(patches)
        return d

    rng = np.random.default_rng(20)
    P = [rng.integers(0, 256, (side, side), dtype=np.uint8)]
    dP, B, dB = [desc(P)[0]], [], []
    while len(B) < n:
        cand = rng.integers(0, 256, (batch, side, side), dtype=np.uint8)
        bl = [_blend(c, P[-1]) for c in cand]
        dc, db = desc(cand), desc(bl)
        for k in range(batch):
            best, second = _hamming(db[k:k + 1], dc[k:k + 1])[0, 0], _hamming(db[k:k + 1], dP[-1][None])[0, 0]
            if not (DOMINO_BEST[0] <= best <= DOMINO_BEST[1] and DOMINO_SECOND[0] <= second <= DOMINO_SECOND[1]):
                continue
            if len(dP) > 1 and _hamming(db[k:k + 1], np.array(dP[:-1])).min() < DOMINO_OTHER:
                continue
            if dB and _hamming(dc[k:k + 1], np.array(dB)).min() < DOMINO_OTHER:
                continue
            P.append(cand[k]); dP.append(dc[k]); B.append(bl[k]); dB.append(db[k])
            break
    spare = []
    while len(spare) < n_spare:
        cand = rng.integers(0, 256, (batch, side, side), dtype=np.uint8)
        dc = desc(cand)
        far = (_hamming(dc, np.array(dP)).min(1) >= DOMINO_OTHER) & (_hamming(dc, np.array(dB)).min(1) >= DOMINO_OTHER)
        spare += [cand[k] for k in np.flatnonzero(far)][:n_spare - len(spare)]
    return np.array(P), np.array(B), np.array(spare)


@functools.lru_cache(maxsize=None)
def domino_scene(name):
    """(params, frames, info): frames = [(L, R, corners_left, corners_right)] for track_with_external_corners; info = dict(n_chain, chain = corner
    indices of the chain's nodes in chain order, n_corners).

    `chain_across_super_chunks` orders its corners: first half of the chain, dense fillers (pitch 16: ~44 candidates each within the radius), sparse
    fillers (pitch 28: ~14), second half of the chain, spares.  The dense fillers fill the 24 576-entry list area, so super-chunk 0 ends among them and
    the head of the second half prefers a target that carries super-chunk 0's permanent mark, not a claim.  The number of sparse fillers is chosen from
    the geometry alone so that the second half starts 24 queries in front of local index 1 024 of super-chunk 1: the chain runs out of the threads'
    first queries (threads 1000 .. 1023) into their second ones (threads 0 .. 23).  2048 x 1040 px is what the 843 sparse fillers need; one detection
    cell of 4096 px, the largest a handle takes."""
    W, H, (lc, lr, lx, ly), dense, sparse, staged, n_frames = DOMINO_SCENES[name]
    nodes = boustrophedon(lc, lr, lx, ly)
    n = len(nodes)
    prm = lvt_amd.kitti_params(width=W, height=H)
    prm.tracking_radius, prm.staged_threshold, prm.triangulation_policy = DOMINO_RADIUS, staged, 2
    prm.tracking_ratio_test_threshold = prm.triangulation_ratio_test_threshold = DOMINO_RATIO
    if W > 1241:          # detection is unused: one cell for the large image (the KITTI-sized scene keeps KITTI's grid: its parameters serve the ordinary
        prm.detection_cell_size = 4096          # world that shares the lock-step pool with it)
    # one spare corner behind every lattice row, on the background and last in the corner order: the last query of a chain still has two candidates to
    # choose from (with one left, the absolute threshold would decide, and reject)
    spare = np.array([(lx + DOMINO_PITCH * lc, ly + DOMINO_PITCH * r) for r in range(lr)], dtype=np.int64)
    if dense is None:
        corners, chain = np.vstack([nodes, spare]), np.arange(n)
    else:
        dc, dr, dx, dy, dp = dense
        D = np.array([(dx + dp * c, dy + dp * r) for r in range(dr) for c in range(dc)], dtype=np.int64)
        sc, sx, sy, sp = sparse
        half = n // 2
        head = np.vstack([nodes[:half], D])
        # the cut of super-chunk 0 from the geometry: candidates of a map point = corners closer than the radius (fillers and nodes are > radius apart)
        cnt = np.concatenate([_neighbour_counts(nodes.astype(np.float64), DOMINO_RADIUS)[:half], _neighbour_counts(D.astype(np.float64), DOMINO_RADIUS)])
        first = super_chunks(cnt)[0][1]
        assert half < first < len(head), (first, len(head))
        n_sparse = RES_THREADS - 24 - (len(head) - first)
        S = np.array([(sx + sp * (k % sc), sy + sp * (k // sc)) for k in range(n_sparse)], dtype=np.int64)
        assert S[:, 1].max() < H - DOMINO_HALF - 1 and S[:, 0].max() < W - DOMINO_HALF - 1
        corners = np.vstack([head, S, nodes[half:], spare])
        chain = np.concatenate([np.arange(half), len(head) + n_sparse + np.arange(n - half)])
    P, blend, spare_patches = domino_patches(n, lr)
    back = np.random.default_rng(21).integers(0, 256, (H, W), dtype=np.uint8)

    def paste(img, patches, shift):
        for (x, y), p in list(zip(nodes, patches)) + list(zip(spare, spare_patches)):
            img[y - DOMINO_HALF:y + DOMINO_HALF + 1, x - shift - DOMINO_HALF:x - shift + DOMINO_HALF + 1] = p
        return np.ascontiguousarray(img)

    L0 = paste(back.copy(), P[:-1], 0)
    R0 = paste(np.roll(back, -DOMINO_DISP, axis=1), blend, DOMINO_DISP)
    L1 = paste(back.copy(), blend, 0)
    R1 = np.ascontiguousarray(np.roll(L1, -DOMINO_DISP, axis=1))
    cl = corners.astype(np.float64)
    cr = cl - [[float(DOMINO_DISP), 0.0]]
    frames = [(L0, R0, cl, cr)] + [(L1, R1, cl, cr)] * (n_frames - 1)
    if name == "staged_chain":
        fill = cl[half:len(head) + n_sparse]
        keep = np.r_[0:len(cl) - lr, len(cl) - lr + STAGED_CHAIN_DROPPED:len(cl)]
        frames = [(L0, R0, fill, fill - [[float(DOMINO_DISP), 0.0]]), (L0, R0, cl, cr), (L1, R1, cl[keep], cr[keep])]
    return prm, frames, dict(n_chain=n, chain=chain, n_corners=len(corners))


# ---- the two procedures over explicit candidate lists ------------------------------------------------------------------------------------------------
# A list holds a query's candidates as (distance, target index) sorted ascending; accept is accept_match's rule (k_track.hip; find_match_index and
# row_match in the oracle): with two or more candidates available the ratio of the best two distances decides (in fp32, 0 / 0 rejects), with exactly
# one the absolute threshold.
def _accept(avail, ratio, desc_th):
    if len(avail) > 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            return bool(np.float32(avail[0][0]) / np.float32(avail[1][0]) < np.float32(ratio))
    return len(avail) == 1 and np.float32(avail[0][0]) <= np.float32(desc_th)


def greedy_serial(lists, ratio, desc_th, marked=()):
    """(a) the reference's scan: query q takes the best of its still unmarked candidates if the rule accepts it, and marks it.  Returns the
    decisions (target or -1)."""
    marked = set(marked)
    out = []
    for lst in lists:
        avail = [c for c in lst if c[1] not in marked][:2]
        out.append(avail[0][1] if _accept(avail, ratio, desc_th) else -1)
        if out[-1] >= 0:
            marked.add(out[-1])
    return out


def greedy_fixpoint(lists, ratio, desc_th, marked=()):
    """(b) the synchronous fixpoint: in iteration t every query decides at once; a candidate is unavailable when it is marked or when a query with a
    smaller index accepted it in iteration t - 1.  Ends with the first iteration that changes no decision.  Returns (decisions, iterations)."""
    marked = set(marked)
    prev, claim, it = [-2] * len(lists), {}, 0
    while True:
        it += 1
        cur, new_claim = [], {}
        for q, lst in enumerate(lists):
            avail = [c for c in lst if c[1] not in marked and claim.get(c[1], q) >= q][:2]
            d = avail[0][1] if _accept(avail, ratio, desc_th) else -1
            cur.append(d)
            if d >= 0 and d not in new_claim:
                new_claim[d] = q            # (queries come in ascending order: the first claim is the earliest query's)
        if cur == prev:
            return cur, it
        prev, claim = cur, new_claim


def _hamming(a, b):
    return np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(2).astype(np.int64)


def map_lists(prm, map_xyz, map_desc, q, p, feat_xy, feat_desc):
    """find_matches' candidate lists: map points projected with the pose (q = w x y z, p: camera to world), features closer than the tracking radius
    (find_match_index's fp32 test; its hash cells cover the circle).  Returns (lists, visible)."""
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    Xc = (map_xyz - p) @ R
    vis = (Xc[:, 2] >= prm.near_plane_distance) & (Xc[:, 2] <= prm.far_plane_distance)
    zc = np.where(vis, Xc[:, 2], 1.0)
    u, v = prm.fx * Xc[:, 0] / zc + prm.cx, prm.fy * Xc[:, 1] / zc + prm.cy
    vis &= (u >= 0) & (u <= prm.img_width) & (v >= 0) & (v <= prm.img_height)
    dx = feat_xy[None, :, 0] - u.astype(np.float32)[:, None]
    dy = feat_xy[None, :, 1] - v.astype(np.float32)[:, None]
    near = (dx * dx + dy * dy) < np.float32(prm.tracking_radius * prm.tracking_radius)
    lists = []
    for i in range(len(map_xyz)):
        idx = np.flatnonzero(near[i]) if vis[i] else np.zeros(0, np.int64)
        d = _hamming(map_desc[i:i + 1], feat_desc[idx])[0] if len(idx) else []
        lists.append(sorted(zip((int(k) for k in d), (int(k) for k in idx))))
    return lists, vis


def row_lists(left_xy, left_desc, right_xy, right_desc, img_rows):
    """row_match's candidate lists: every right feature of the query's +-2 row band, whatever its x"""
    lists = []
    for i in range(len(left_xy)):
        y0, y1 = max(int(left_xy[i, 1]) - 2, 0), min(int(left_xy[i, 1]) + 2, img_rows)
        idx = np.flatnonzero((right_xy[:, 1] >= y0) & (right_xy[:, 1] <= y1))
        d = _hamming(left_desc[i:i + 1], right_desc[idx])[0] if len(idx) else []
        lists.append(sorted(zip((int(k) for k in d), (int(k) for k in idx))))
    return lists


# ---- RGB-D at its depth and lens edges ---------------------------------------------------------------------------------------------------------------
# What only an RGB-D frame reaches: the depth lookup and the near / far filter of k_gather, its 16-bit conversion, undistort_point with the "left the
# hash grid -> drop" rule, the fp32 back-projection of k_triangulate.  All cases are the synthetic TUM world of seed 1 at 640 x 480.
RGBD_EDGE_SEED = 1
RGBD_NEAR, RGBD_FAR = 0.5, 5.0
RGBD_GATES = {"near_plane_distance": RGBD_NEAR, "far_plane_distance": RGBD_FAR}
RGBD_PLANT_FRAMES = 4           # frame 0 with the planted plane, frames 1 - 3 with the world's own depth
# 16-bit sets: (depth_scale, raw classes).  Each decides one gate by the rounding of the fp32 product alone (checked over all 65536 raws: the fp32 and
# the float64 product disagree about the gates at raw 2500 of set A and at raw 5000 of set B, nowhere else):
#   A  raw 2500: fp32 product exactly 0.5 = near, kept; the exact product of the two fp32 operands is 0.49999998..., below near
#   B  raw 5000: fp32 product exactly 5.0 = far, kept; the exact product is 5.0000002..., above far (and raw / (1f / scale) = 5.0000005)
#      raw 500: fp32 product exactly 0.5 = near; the exact product lies above it, so the gate keeps it either way -- what raw 500 pins is the value:
#      raw / (1f / scale) gives 0.50000006, another map point
RGBD16_SETS = {
    "A": (np.float32(1) / np.float32(5000), (0, 1, 2499, 2500, 2501, 12345, 24999, 25000, 25001, 65535)),
    "B": (np.float32(0.001), (0, 499, 500, 501, 4999, 5000, 5001, 65535)),
}
RGBD16_FRAMES = 3
# barrel distortion (k1 < 0: the sign of RealSense / Kinect-class colour cameras; these are the EuRoC cam0 coefficients).  Measured with the oracle on
# seed 1, frames 0 - 7 (test_case_tables.py asserts the conditions): TRACKING throughout, 683 - 798 matches from frame 1, 7 - 11 features kept outside
# the image per frame (x up to 649.7), 10 - 22 corners dropped for leaving the hash grid, and 3 - 7 find_matches matches per frame from frame 1 (36 in
# all) that land on a feature outside the image -- so seed 1 serves, no other seed was needed
RGBD_BARREL = dict(k1=-0.28340811, k2=0.07395907, p1=0.00019359, p2=1.76187114e-05, k3=0.0)
RGBD_BARREL_FRAMES = 8
RGBD_RETRY = {"agast_threshold": 150}       # 159 - 181 corners per frame: below the 200 that send the image through the detector again
RGBD_RETRY_FRAMES = 4
# scripts of frames without valid depth: name -> (depth kinds per frame, the oracle's status per frame).  "world": the world's depth; "nan": an
# all-NaN fp32 plane; "zero": an all-zero fp32 plane; "zero16": a uint16 plane of raw 0 (the oracle gets fp32 zeros)
RGBD_NODEPTH = {
    "nan_first": (("nan", "world", "world"), (2, 3, 3)),
    "zero_mid": (("world", "world", "zero", "world"), (2, 2, 3, 3)),
    "zero16_mid": (("world", "world", "zero16", "world"), (2, 2, 3, 3)),
}


def rgbd_depth_classes(near=RGBD_NEAR, far=RGBD_FAR):
    """the 15 fp32 depth values planted at the corners: what no rendered depth plane holds.  Kept by `near <= d <= far` in fp32: classes 8 - 12."""
    n, f, lo, hi = np.float32(near), np.float32(far), np.float32(-np.inf), np.float32(np.inf)
    return np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1e-45, np.nextafter(n, lo), n, np.nextafter(n, hi), 1.5,
                     np.nextafter(f, lo), f, np.nextafter(f, hi), 3.4e38], dtype=np.float32)


def rgbd_world(overrides=None):
    from parity_util import make_case
    world, prm, sensor = make_case("tum", RGBD_EDGE_SEED, 1.0, overrides)
    assert sensor == 2 and (world.W, world.H) == (640, 480)
    return world, prm


@functools.lru_cache(maxsize=None)
def rgbd_planted(kind):
    """kind "f32": frame 0 of the world under RGBD_GATES with class i % 15 of rgbd_depth_classes() written into the depth plane at corner i of
    O.compute_features(gray) (list order; the corners are integer and distinct); kind "A" / "B": a uint16 plane (the world's depth in raw units) with
    raw class i % len(raws) of that 16-bit set.  Returns a dict: prm, scale (None for f32), frames = [(gray, depth plane as handed in, its fp32 value
    as the oracle gets it)] -- the planted frame, then the world's own frames --, xy / desc = the corner list, val = the fp32 depth at every corner,
    keep = near <= val <= far in numpy float32."""
    from oracle import pyoracle as O
    world, prm = rgbd_world(RGBD_GATES)
    n_frames = RGBD_PLANT_FRAMES if kind == "f32" else RGBD16_FRAMES
    rendered = [world.render_rgbd(i) for i in range(n_frames)]
    gray = np.ascontiguousarray(rendered[0][0])
    xy, _, desc, retry = O.compute_features(gray, prm)
    assert retry == 0 and np.array_equal(xy, np.rint(xy)) and len(np.unique(xy, axis=0)) == len(xy)
    ix, iy = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
    if kind == "f32":
        scale = None
        cls = rgbd_depth_classes()
        val = cls[np.arange(len(xy)) % len(cls)]
        plane = np.array(rendered[0][1], dtype=np.float32)
        plane[iy, ix] = val
        frames = [(gray, plane, plane)] + [(np.ascontiguousarray(g), np.ascontiguousarray(d, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32))
                                           for g, d in rendered[1:]]
    else:
        scale, raws = RGBD16_SETS[kind]
        raws = np.array(raws, dtype=np.uint16)

        def to_raw(d):
            return np.clip(np.rint(d.astype(np.float64) / np.float64(scale)), 0, 65535).astype(np.uint16)
        u = to_raw(rendered[0][1])
        u[iy, ix] = raws[np.arange(len(xy)) % len(raws)]
        us = [u] + [to_raw(d) for _, d in rendered[1:]]
        frames = []
        for (g, _), uu in zip(rendered, us):
            f = uu.astype(np.float32) * scale           # ONE rounded fp32 multiply
            assert f.dtype == np.float32
            frames.append((np.ascontiguousarray(g), uu, f))
        val = frames[0][2][iy, ix]
    with np.errstate(invalid="ignore"):
        keep = (val >= np.float32(prm.near_plane_distance)) & (val <= np.float32(prm.far_plane_distance))
    return dict(prm=prm, scale=scale, frames=frames, xy=xy, desc=desc, val=val, keep=keep)


def rgbd_backproject(prm, uv, z):
    """k_triangulate's RGB-D branch (lvt_local_map.cpp:231-256) under the identity pose, restated in numpy float32 and widened: x = (u - cx) z (1f / fx),
    y = (v - cy) z (1f / fy), z.  The fp64 rotation of the first frame multiplies by exact ones and adds exact zeros."""
    f = np.float32
    u, v, z = uv[:, 0].astype(f), uv[:, 1].astype(f), z.astype(f)
    x = (u - f(prm.cx)) * z * (f(1) / f(prm.fx))
    y = (v - f(prm.cy)) * z * (f(1) / f(prm.fy))
    assert x.dtype == np.float32 and y.dtype == np.float32
    return np.column_stack([x, y, z]).astype(np.float64)


def rgbd_outside(xy, W=640, H=480):
    """features kept although they left the image: the hash grid reaches to 25 ceil(W / 25) x 25 ceil(H / 25)"""
    return (xy[:, 0] >= W) | (xy[:, 1] >= H) | (xy[:, 0] < 0) | (xy[:, 1] < 0)


def rgbd_nodepth_script(name):
    """(prm, [(gray, depth plane as handed in, its fp32 value), ...], the oracle's status per frame) of one RGBD_NODEPTH script"""
    world, prm = rgbd_world()
    kinds, status = RGBD_NODEPTH[name]
    frames = []
    for i, kind in enumerate(kinds):
        g, d = world.render_rgbd(i)
        g, d = np.ascontiguousarray(g), np.ascontiguousarray(d, dtype=np.float32)
        if kind == "nan":
            d = np.full_like(d, np.nan)
        elif kind in ("zero", "zero16"):
            d = np.zeros_like(d)
        frames.append((g, np.zeros(d.shape, np.uint16) if kind == "zero16" else d, d))
    return prm, frames, status


# ---- turns past 180 degrees --------------------------------------------------------------------------------------------------------------------------
# The synthetic worlds of lvt_amd/synth.py turn by a few degrees, so every other sequence keeps its pose quaternion at w > 0.99.  These cases drive the
# tracker through half a turn and more (turn_worlds.py): the published pose flips from q to -q between two frames (k_pnp keeps w >= 0), motion_predict takes
# the d < 0 arm of its slerp and predicts a pose with w < 0, the rotation matrices leave the identity (R[0] < 0: the right camera towards the world's -x),
# and -- in the room with culling switched off -- hundreds of map points lie behind the camera and project inside the image with a negative depth.
# Measured with the oracle (test_case_tables.py asserts the conditions; half-size KITTI is 620 x 188, half-size TUM 320 x 240):
#   roll_past_180    TRACKING on all 76 frames, pose w down to 0.0092 at frame 60, predicted w < 0 at frames 60 and 61 (-0.0094, -0.0348)
#   room_loop        TRACKING on all 150 frames, |w| down to 0.0044 at frame 73, predicted w < 0 at frames 73 and 74, at most 1 point behind the camera
#   room_loop_keep   TRACKING on all 150 frames, |w| down to 0.0021, the map grows to 2 040 points, up to 1 008 of them behind the camera, up to 518 of those
#                    inside the image; 100 or more of them on 108 frames
#   room_rgbd        (3 m room, radius 0.8 m, 2 degrees per frame, 0.01 m texels) TRACKING on all 100 frames, |w| down to 0.0081 at frame 91
# name: (world kind, world parameters, parameter overrides, frames, sensor)
TURN_CASES = {
    "roll_past_180": ("roll", dict(deg_per_frame=3.0), {}, 76, 1),
    "room_loop": ("room", dict(deg_per_frame=2.5, radius=3.0), {}, 150, 1),
    "room_loop_keep": ("room", dict(deg_per_frame=2.5, radius=3.0), {"untracked_threshold": 1000}, 150, 1),
    "room_rgbd": ("room", dict(deg_per_frame=2.0, radius=0.8, half_side=3.0, texel=0.01), {}, 100, 2),
}
TURN_MIN_ABS_W = 1e-3             # below it the sign of w would be a matter of rounding
TURN_KEEP_FRAMES, TURN_KEEP_POINTS = 100, 100     # room_loop_keep: on so many frames so many points are kept out by the near plane alone
TURN_CULLED_POINTS = 5            # room_loop (default culling): never more than this handful

_TURN_WORLDS = {}


def turn_case(name):
    """(world, params, sensor, frames) of one TURN_CASES entry.  Worlds are kept (and keep their frames): room_loop and room_loop_keep share one."""
    from parity_util import make_case
    from turn_worlds import RolledWorld, RoomWorld
    kind, wkw, overrides, n, sensor = TURN_CASES[name]
    base, prm, s = make_case("kitti" if sensor == 1 else "tum", 0, 0.5, overrides)
    assert s == sensor
    key = (kind, sensor, tuple(sorted(wkw.items())))
    if key not in _TURN_WORLDS:
        if kind == "roll":
            _TURN_WORLDS[key] = RolledWorld(base, **wkw)
        else:
            _TURN_WORLDS[key] = RoomWorld(base.W, base.H, base.fx, base.fy, base.cx, base.cy, base.baseline, seed=0, **wkw)
    return _TURN_WORLDS[key], prm, sensor, n


def quat_to_R(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def behind_camera_in_image(prm, xyz, q, p, near_gate=True):
    """the number of map points that is_point_visible's `cz < near_plane` ALONE keeps out of the match lists, with cz < 0: under the pose (q = w x y z, p:
    camera to world) they lie behind the camera, yet projected with inv_z = 1 / cz they land inside [0, W) x [0, H), and the far plane passes every negative
    depth.  near_gate=False restates the gate without that comparison: nothing is kept out then, the count is zero."""
    if not len(xyz):
        return 0
    Xc = (np.asarray(xyz) - p) @ quat_to_R(q)
    cz = Xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = prm.fx * Xc[:, 0] / cz + prm.cx, prm.fy * Xc[:, 1] / cz + prm.cy
        inside = (u >= 0) & (u < prm.img_width) & (v >= 0) & (v < prm.img_height)
    without = inside & ~(cz > prm.far_plane_distance)
    with_gate = without & ~(cz < prm.near_plane_distance) if near_gate else without
    return int((without & ~with_gate & (cz < 0)).sum())


# ---- the motion model alone: the branches of motion_predict (lvt_math.h) / MotionModel::predict (the oracle) no sequence reaches ------------------------
MOTION_ONE = 1.0 - 2.0 ** -52       # Eigen's slerp: at |d| >= 1 - epsilon the weights are (1 - t, t)
MOTION_SMALL_ANGLES = (1e-9, 3e-9, 1e-8, 1.5e-8, 2e-8, 5e-8, 1e-7, 1e-6, 1e-4, 1e-2)     # cos a walks through MOTION_ONE between 2e-8 and 5e-8
MOTION_RANDOM = 200


def _axis_angle(axis, a):
    axis = np.asarray(axis, float)
    return np.array([np.cos(a / 2), *(np.sin(a / 2) * axis / np.linalg.norm(axis))])


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def motion_edge_cases():
    """[(label, state[14] = last_q, ang_vel, last_p, lin_vel, q[4], p[3])].  last_q is the identity unless the label says otherwise, so diff = cur.q * last_q^-1
    is cur.q exactly and d = diff . ang_vel is known in advance."""
    ident = np.array([1.0, 0, 0, 0])
    rows = []

    def add(label, q, last_q=ident, ang_vel=ident, p=(0.3, -0.2, 1.5), last_p=(0.1, 0.1, 1.0), lin_vel=(0.15, -0.25, 0.45)):
        rows.append((label, np.concatenate([last_q, ang_vel, last_p, lin_vel]).astype(np.float64), np.asarray(q, np.float64), np.asarray(p, np.float64)))
    add("stationary", ident, p=(1.0, 2.0, 3.0), last_p=(1.0, 2.0, 3.0), lin_vel=(0, 0, 0))                    # d = 1 exactly, nothing moves
    for a in MOTION_SMALL_ANGLES:
        q = np.array([np.cos(a), np.sin(a), 0, 0])
        add(f"small_{a:g}", q)
        add(f"small_{a:g}_negated_velocity", q, ang_vel=-ident)                                              # d < 0
        add(f"small_{a:g}_negated_pose", -q)                                                                 # d < 0
    add("orthogonal_axes", [0.0, 1, 0, 0])                                                                   # d = +0.0, theta = pi / 2
    c, s = np.cos(0.3), np.sin(0.3)
    add("orthogonal_cancelling", [c, s, 0, 0], ang_vel=np.array([-s, c, 0, 0]))                              # d = -cs + sc = +0.0
    for deg in (90.0, 179.0, 179.999):                                                                      # the angle between diff and ang_vel as 4-vectors
        f = np.deg2rad(deg)
        add(f"wide_{deg:g}", ident, ang_vel=np.array([np.cos(f), 0, np.sin(f), 0]))
        add(f"wide_{deg:g}_rotated", _axis_angle([1, 2, 3], 0.7), ang_vel=_qmul(_axis_angle([1, 2, 3], 0.7), np.array([np.cos(f), 0, np.sin(f), 0])))
    g = _axis_angle([0.2, -1.0, 0.4], 1.1)
    add("zero_last_q", g, last_q=np.zeros(4), ang_vel=_axis_angle([0, 1, 0], 0.2))                          # inv = 0, diff = 0
    add("last_q_norm_3", g, last_q=3.0 * _axis_angle([0.5, 1.0, 0.1], 0.9), ang_vel=_axis_angle([0, 1, 0], 0.2))
    add("last_q_norm_1e-3", g, last_q=1e-3 * _axis_angle([0.5, 1.0, 0.1], 0.9), ang_vel=_axis_angle([0, 1, 0], 0.2))
    add("cur_q_norm_2", 2.0 * g, last_q=_axis_angle([0.5, 1.0, 0.1], 0.9), ang_vel=_axis_angle([0, 1, 0], 0.2))
    add("large_positions", g, p=(1e6, -2e6, 3e6), last_p=(1e6 - 0.5, -2e6 + 0.25, 3e6 - 1.0), lin_vel=(1e6, 1e6, -1e6))
    add("tiny_positions", g, p=(1e-12, -2e-12, 3e-12), last_p=(2e-12, 1e-12, -1e-12), lin_vel=(1e-12, -1e-12, 1e-12))
    rng = np.random.default_rng(20260)
    for k in range(MOTION_RANDOM):
        last_q = _axis_angle(rng.normal(size=3), rng.uniform(0, 2 * np.pi))
        q = _qmul(_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0, 170))), last_q) * rng.choice([-1.0, 1.0])
        av = _axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0, 170))) * rng.choice([-1.0, 1.0])
        last_p = rng.normal(0, 10, 3)
        add(f"random_{k}", q, last_q=last_q, ang_vel=av, p=last_p + rng.normal(0, 1, 3), last_p=last_p, lin_vel=rng.normal(0, 1, 3))
    return rows


MOTION_EDGE_CASES = motion_edge_cases()


def motion_slerp_dot(state, q):
    """(d, |diff|): the dot product motion_predict's slerp branches on, in the code's own operation order (fp64)"""
    lq, b = state[0:4], state[4:8]
    n2 = lq[0] * lq[0] + lq[1] * lq[1] + lq[2] * lq[2] + lq[3] * lq[3]
    inv = np.array([lq[0] / n2, -lq[1] / n2, -lq[2] / n2, -lq[3] / n2]) if n2 > 0 else np.zeros(4)
    diff = _qmul(q, inv)
    return diff[0] * b[0] + diff[1] * b[1] + diff[2] * b[2] + diff[3] * b[3], float(np.linalg.norm(diff))


def motion_predict_longdouble(state, q, p):
    """lvt_motion_model.cpp:42-65 with Eigen 3.3's inverse / slerp / normalize, restated in numpy.longdouble from the fp64 inputs: (next[14], q_out, p_out).
    The slerp's `one` is the fp64 constant of the code, whatever the precision of the arithmetic."""
    L = np.longdouble
    st, q, p = np.asarray(state, L), np.asarray(q, L), np.asarray(p, L)
    lq, b, lp, lv = st[0:4], st[4:8], st[8:11], st[11:14]
    half = L(0.5)
    nv = ((p - lp) + lv) * half
    n2 = (lq * lq).sum()
    inv = np.array([lq[0], -lq[1], -lq[2], -lq[3]], L) / n2 if n2 > 0 else np.zeros(4, L)
    diff = _qmul(q, inv)
    d = (diff * b).sum()
    if abs(d) >= L(MOTION_ONE):
        s0 = s1 = half
    else:
        th = np.arccos(abs(d))
        s0, s1 = np.sin(half * th) / np.sin(th), np.sin(half * th) / np.sin(th)
    if d < 0:
        s1 = -s1
    nav = s0 * diff + s1 * b

    def normalized(x):
        z = (x * x).sum()
        return x / np.sqrt(z) if z > 0 else x
    nav = normalized(nav)
    out_q = normalized(_qmul(q, nav))
    return np.concatenate([q, nav, p, nv]), out_q, p + nv


# ---- the batched Hamming matcher: every template instance, its overflow bounds, its dispatch boundaries (test_gpu_hamming_instances.py) ----------------
# The host's dispatch rule and LDS formula, restated (tools/hamming_sweep.py states the picker as well, but imports torch and opens the device, and keys
# the family by the name of a mask instead of r2).  Restated from lvt_amd/csrc:
#   lvt_host.hip  lvt_amd_hamming_match_batched_n: the size caps (N <= HB_NMAX, M <= HB_MMAX), nbx / nby / csr, the LDS check (the carve-up plus the
#                 kernel's static arrays within a workgroup's 160 KiB), and the picker
#                 (qpt, tpt = ceil(M / HB_THREADS), ceil(N / HB_THREADS); row mode <1,1>, csr 1 <0,3>, csr 2 <0,5>, any other csr <0,0>)
#   k_hamming.hip hamming_lds_bytes, HB_THREADS, HB_TPT, HB_QPT; the chunk of the chunked bin scan (step 2); MASK_BITS and the 64-candidate masks
HB_THREADS = 1024
HB_MMAX = HB_NMAX = 4 * HB_THREADS
HB_LDS_MAX = 160 * 1024
HB_STATIC_LDS = 400                 # s_scan (128 B) + s_hist (256 B) + s_recheck (4 B) as every instance's code object lays them out: the host asks the runtime
HB_MASK_BITS = 41                   # packed csr-1 family: window candidates a query's slot words hold a radius bit for
HB_RANGE_MAX = 63                   # ... and the longest range its 6-bit length fields hold
HB_TWO_STAGE_MAX = 64               # unpacked two-stage family (csr 2): window candidates of the two mask words
HASH_CELL = 25
HAMMING_GEOMETRY = (376, 1241)      # rows, cols of test_every_instance
# family -> (mode, NSP, r2 of test_every_instance)
HAMMING_FAMILIES = {"row": (1, 1, 0.0), "csr1": (0, 3, 625.0), "csr2": (0, 5, 2500.0), "any": (0, 0, 5625.0)}


def hamming_csr(r2):
    """max(1, ceil(sqrt(r2) / 25)) in fp32, as the host computes it"""
    return max(1, int(np.ceil(np.sqrt(np.float32(r2)) / np.float32(HASH_CELL))))


def hamming_grid(mode, rows, cols):
    """(nbx, nby): hash cells in radius mode, one bin per image row 0 .. rows in row mode"""
    if mode == 1:
        return 1, rows + 1
    return int(np.ceil(np.float32(cols) / np.float32(HASH_CELL))), int(np.ceil(np.float32(rows) / np.float32(HASH_CELL)))


def hamming_nbins(mode, rows, cols):
    nbx, nby = hamming_grid(mode, rows, cols)
    return nbx * nby


def hamming_lds_bytes(N, M, nbins):
    """hamming_lds_bytes of k_hamming.hip: 42 N + 14 M (the u16 arrays rounded up to an even count) + 4 (nbins + 1) + 16"""
    return N * 32 + N * 8 + M * 12 + (nbins + 1) * 4 + ((N + 1) & ~1) * 2 + ((M + 1) & ~1) * 2 + 16


def hamming_lds_fits(N, M, nbins):
    return hamming_lds_bytes(N, M, nbins) + HB_STATIC_LDS <= HB_LDS_MAX


def hamming_instance(mode, r2, M, N):
    """<MODE, NSP, QPT, TPT> of the launch"""
    qpt, tpt = -(-M // HB_THREADS), -(-N // HB_THREADS)
    if mode == 1:
        return (1, 1, qpt, tpt)
    csr = hamming_csr(r2)
    return (0, {1: 3, 2: 5}.get(csr, 0), qpt, tpt)


def hamming_admitted(mode, M, N, rows, cols):
    """the entry launches: sizes within the caps and the LDS need within 160 KiB"""
    return 0 < M <= HB_MMAX and 0 < N <= HB_NMAX and hamming_lds_fits(N, M, hamming_nbins(mode, rows, cols))


def hamming_scan_chunk(nbins):
    """entries per thread of the bin scan: 0 = one entry per thread (nbins + 1 <= HB_THREADS), else the chunked scan's ceil((nbins + 1) / HB_THREADS)"""
    return 0 if nbins + 1 <= HB_THREADS else -(-(nbins + 1) // HB_THREADS)


def _hamming_instance_table():
    """per family and (QPT, TPT) class the smallest member (M, N) = (1024 (q - 1) + 1, 1024 (t - 1) + 1) and the largest one: M = 1024 q with N = 1024 t
    lowered to the largest the LDS bound admits; where that N would leave the class (the bound is 42 N + 14 M: only at (3, 4)), N stays the smallest of
    the class and M is lowered instead.  A class whose smallest member the bound refuses has no member at all."""
    rows, cols = HAMMING_GEOMETRY
    table = []
    for fam, (mode, _, r2) in HAMMING_FAMILIES.items():
        nb = hamming_nbins(mode, rows, cols)
        fits = lambda M, N: hamming_lds_fits(N, M, nb)
        for q in range(1, 5):
            for t in range(1, 5):
                m0, n0 = HB_THREADS * (q - 1) + 1, HB_THREADS * (t - 1) + 1
                if not fits(m0, n0):
                    continue
                table.append((fam, q, t, "smallest", m0, n0))
                m1 = HB_THREADS * q
                if fits(m1, n0):
                    n1 = max(n for n in range(n0, HB_THREADS * t + 1) if fits(m1, n))
                else:
                    n1 = n0
                    m1 = max(m for m in range(m0, m1 + 1) if fits(m, n0))
                table.append((fam, q, t, "largest", m1, n1))
    return table


HAMMING_INSTANCE_CASES = _hamming_instance_table()


def hamming_window_counts(qxy, txy, tf, csr, rows, cols):
    """(M, 2 csr + 1) int: unflagged train features in each row of a query's window of hash cells -- the kernel's candidate ranges (l_0 .. l_2csr).
    Cells are floor(x / 25) in fp32, clamped into the grid for a feature, the window clipped to the grid for a query (struct.cpp:71-83)."""
    nbx, nby = hamming_grid(0, rows, cols)
    cell = lambda v: np.floor(v.astype(np.float32) / np.float32(HASH_CELL)).astype(np.int64)
    keep = tf == 0
    tcx, tcy = np.clip(cell(txy[keep, 0]), 0, nbx - 1), np.clip(cell(txy[keep, 1]), 0, nby - 1)
    grid = np.zeros((nby, nbx + 1), np.int64)
    np.add.at(grid, (tcy, tcx + 1), 1)
    cum = np.cumsum(grid, axis=1)                                         # cum[y, x] = features of row y in cells < x
    hx, hy = cell(qxy[:, 0]), cell(qxy[:, 1])
    x0, x1 = np.maximum(hx - csr, 0), np.minimum(hx + csr, nbx - 1)
    y0, y1 = np.maximum(hy - csr, 0), np.minimum(hy + csr, nby - 1)
    out = np.zeros((len(qxy), 2 * csr + 1), np.int64)
    for k in range(2 * csr + 1):
        ok = (y0 + k <= y1) & (x0 <= x1)
        yy = np.where(ok, y0 + k, 0)
        out[:, k] = np.where(ok, cum[yy, np.where(ok, x1 + 1, 0)] - cum[yy, np.where(ok, x0, 0)], 0)
    return out


@functools.lru_cache(maxsize=4)
def hamming_instance_problem(fam, M, N):
    """the two problems of one case of test_every_instance: (qd, qxy, td, txy, tf), B = 2.
    0: uniform integer features and a strip of graded density, about 15 % flagged, descriptors from 8 prototypes (ties resolve by the lowest index),
       queries outside the image on all four sides;
    1: half the features and queries in a dense 120 x 90 cluster (windows past 64 candidates, ranges past 63: the in-place match_all fallbacks); in row
       mode fractional / out-of-range / NaN rows, which send this problem -- and not the other -- through the comparing walk."""
    mode = HAMMING_FAMILIES[fam][0]
    rows, cols = HAMMING_GEOMETRY
    rng = np.random.default_rng([M, N, mode, HAMMING_FAMILIES[fam][1]])
    B = 2
    td = rng.integers(0, 256, (B, N, 32), dtype=np.uint8)
    qd = rng.integers(0, 256, (B, M, 32), dtype=np.uint8)
    proto = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    td[0], qd[0] = proto[rng.integers(0, 8, N)], proto[rng.integers(0, 8, M)]
    txy = np.floor(rng.uniform(0, 1, (B, N, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    qxy = (rng.uniform(0, 1, (B, M, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    outside = np.array([[-30.5, 100.25], [cols + 40.0, 100.0], [300.0, -30.5], [300.5, rows + 30.0], [-3.0, -3.0], [cols + 1.0, rows + 1.0],
                        [cols - 0.5, rows - 0.5], [0.0, 0.0], [-200.0, 50.0], [cols + 200.0, 300.0], [600.0, -150.0], [600.0, rows + 150.0]], np.float32)
    k = min(M, len(outside))
    qxy[0, M - k:] = outside[:k]
    ng, mg = N // 8, M // 4             # a strip whose density grows to the right: windows of every size up to the fallbacks'
    txy[0, :ng] = np.floor(np.column_stack([700 + 250 * np.sqrt(rng.uniform(0, 1, ng)), 200 + 75 * rng.uniform(0, 1, ng)])).astype(np.float32)
    qxy[0, :mg] = np.column_stack([rng.uniform(700, 950, mg), rng.uniform(200, 275, mg)]).astype(np.float32)
    nc, mc = N // 2, M // 2
    txy[1, :nc] = np.floor(rng.uniform(0, 1, (nc, 2)) * [120, 90] + [300, 100]).astype(np.float32)
    qxy[1, :mc] = (rng.uniform(0, 1, (mc, 2)) * [120, 90] + [300, 100]).astype(np.float32)
    if mode == 1 and N >= 8:
        j = rng.permutation(N)
        n8 = max(N // 8, 1)
        txy[1, j[:n8], 1] += rng.uniform(0.01, 0.99, n8).astype(np.float32)                    # fractional
        txy[1, j[n8:n8 + 3], 1] = np.array([-4.5, rows + 0.5, rows + 7.0], np.float32)         # above the image (bin 0), below it (last bin)
        txy[1, j[n8 + 3], 1] = np.float32(np.nan)
        txy[1, j[n8 + 4], 1] = np.float32(rows)                                                # the row `end_y` may reach
    tf = (rng.uniform(0, 1, (B, N)) < 0.15).astype(np.uint8)
    for a in (qd, qxy, td, txy, tf):
        a.setflags(write=False)
    return qd, qxy, td, txy, tf


# -- the overflow bounds of the two-stage families: populations with an exact number of window candidates
HAMMING_COUNT_KS = (31, 32, 33, 40, 41, 42, 63, 64, 65)      # the lo | hi mask words, MASK_BITS, the 6-bit range length and the two-word mask
HAMMING_COUNT_GEOMETRY = (350, 1750)                          # 14 x 70 cells = 980 bins: the scan's one-entry-per-thread arm
_COUNT_QUERY_OFFSETS = np.array([[0.0, 0.0], [2.0, -1.5], [-2.5, 1.0], [1.5, 2.5]])      # inside the centre cell; the first is the cell's centre
_COUNT_MARGIN = 3.0                                           # a "robust" feature lies this far inside / outside the circle of EVERY query of its population


def _count_rows(csr, k, layout):
    """{window row j: features}: 'one' = all k in the centre row (one range); 'split' = over all 2 csr + 1 rows -- evenly below 63, and from 63 on one in
    each outer row and the rest in the centre, so that a single range holds k - 2 csr (csr 1: 61 .. 64 for k = 63 .. 66)"""
    if layout == "one":
        return {0: k}
    rows = list(range(-csr, csr + 1))
    if k >= 63:
        per = {j: 1 for j in rows}
        per[0] = k - 2 * csr
    else:
        per = {j: k // len(rows) for j in rows}
        per[0] += k - sum(per.values())
    return per


@functools.lru_cache(maxsize=4)
def hamming_count_case(csr):
    """test_candidate_count_bounds, radius 25 csr: B = 2 problems of the same populations (other descriptors, other positions drawn).  A population owns
    the (2 csr + 1)^2 cells around its centre cell, two empty cells wide all round; its queries sit in the centre cell and see exactly k window
    candidates, about half of them inside the circle, some at distance^2 == r2 exactly from the query at the cell's centre (coordinates are multiples of
    0.5: every square and sum is exact in fp32).  The LAST populated cell of every window row holds one feature, inside the circle of all the population's
    queries: the last candidate of a range is a hit whatever order a cell's features took.  Every feature has a query with its descriptor, one bit flipped.
    Returns (qd, qxy, td, txy, tf, pops): pops = [(k, layout, {row: count}, query indices)]."""
    rows_img, cols_img = HAMMING_COUNT_GEOMETRY
    nbx, nby = hamming_grid(0, rows_img, cols_img)
    r = 25.0 * csr
    pitch = 2 * csr + 3
    slots = [(csr + pitch * i, csr + pitch * j) for j in range((nby - 2 * csr - 1) // pitch + 1) for i in range((nbx - 2 * csr - 1) // pitch + 1)]
    plan = [(k, "one") for k in HAMMING_COUNT_KS] + [(k, "split") for k in HAMMING_COUNT_KS + (66,)]
    assert len(plan) <= len(slots)
    exact = {(a * csr * s, b * csr * t) for a, b in ((25, 0), (0, 25), (7, 24), (24, 7), (15, 20), (20, 15)) for s in (1, -1) for t in (1, -1)}
    out = []
    for b in range(2):
        rng = np.random.default_rng([csr, b, 77])
        txy, qxy, owner = [], [], []
        pops = []
        for (k, layout), (cx, cy) in zip(plan, slots):
            centre = np.array([cx * 25 + 12.5, cy * 25 + 12.5])
            per = _count_rows(csr, k, layout)
            first_q = len(qxy)
            for j, n in per.items():
                dx, dy = np.meshgrid(np.arange(-(r + 12), r + 12.5, 0.5), 25 * j + np.arange(-12, 12.5, 0.5))
                dx, dy = dx.ravel(), dy.ravel()
                d2 = dx * dx + dy * dy
                col = np.floor((12.5 + dx) / 25)
                rin, rout = d2 <= (r - _COUNT_MARGIN) ** 2, d2 >= (r + _COUNT_MARGIN) ** 2
                ex = np.array([(x, y) in exact for x, y in zip(dx, dy)]) & (d2 == r * r)
                cl = col[rin].max()
                pick = [int(rng.choice(np.flatnonzero(rin & (col == cl))))]                     # the last cell's one feature
                rest = n - 1
                e = np.flatnonzero(ex & (col < cl))
                e = rng.permutation(e)[:min(len(e), rest // 4)]
                n_in = (rest - len(e)) // 2
                pick += list(e) + list(rng.choice(np.flatnonzero(rin & (col < cl)), n_in, replace=False))
                pick += list(rng.choice(np.flatnonzero(rout & (col < cl)), rest - len(e) - n_in, replace=False))
                assert len(set(pick)) == n
                for i in pick:
                    txy.append(centre + [dx[i], dy[i]])
                    qxy.append(centre + _COUNT_QUERY_OFFSETS[(len(qxy) - first_q) % 4])
            pops.append((k, layout, per, np.arange(first_q, len(qxy))))
        N = len(txy)
        order = rng.permutation(N)                                                              # train index != construction order
        td = rng.integers(0, 256, (N, 32), dtype=np.uint8)
        qd = np.empty((N, 32), np.uint8)
        t_arr = np.empty((N, 2), np.float32)
        for i, slot in enumerate(order):
            t_arr[slot] = txy[i]
            qd[i] = td[slot]
            qd[i, i % 32] ^= np.uint8(1 << (i % 8))
        out.append((qd, np.array(qxy, np.float32), td, t_arr, np.zeros(N, np.uint8), pops))
    assert [p[:3] for p in out[0][5]] == [p[:3] for p in out[1][5]]
    stack = lambda i: np.stack([out[0][i], out[1][i]])
    return stack(0), stack(1), stack(2), stack(3), stack(4), out[0][5]


# -- the dispatch boundaries in r2
_F32 = np.float32
HAMMING_R2_BOUNDARIES = [(_F32(0.0), "csr1"), (_F32(1e-3), "csr1"), (_F32(625.0), "csr1"), (np.nextafter(_F32(625.0), _F32(np.inf)), "csr2"),
                         (_F32(2500.0), "csr2"), (np.nextafter(_F32(2500.0), _F32(np.inf)), "any"), (_F32(40000.0), "any")]
HAMMING_RING_OFFSETS = [(0, 0), (25, 0), (0, 25), (-25, 0), (0, -25), (7, 24), (-24, 7), (15, -20), (-20, -15),
                        (50, 0), (0, -50), (14, 48), (-48, 14), (30, 40), (-40, -30)]
HAMMING_RING_QUERIES = 60


@functools.lru_cache(maxsize=1)
def hamming_boundary_problem():
    """one problem pair (M, N) = (600, 1200) on 1241 x 376 for every r2 of HAMMING_R2_BOUNDARIES: random integer features, and around each of the first 60
    queries (at multiples of 0.5 px) one feature ON the query, eight at distance 25 exactly and six at 50 exactly (axes, 7-24-25, 15-20-25 and their
    doubles): the strict `<` decides them while the family switches.  A ring feature's descriptor is its query's with 3, 6, 9 .. bits flipped in an order
    drawn per query, so the record names exactly the accepted ones."""
    rows, cols = HAMMING_GEOMETRY
    B, M, N = 2, 600, 1200
    rng = np.random.default_rng(2500)
    td = rng.integers(0, 256, (B, N, 32), dtype=np.uint8)
    qd = rng.integers(0, 256, (B, M, 32), dtype=np.uint8)
    txy = np.floor(rng.uniform(0, 1, (B, N, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    qxy = (rng.uniform(0, 1, (B, M, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    nr = len(HAMMING_RING_OFFSETS)
    for b in range(B):
        slots = rng.permutation(N)[:HAMMING_RING_QUERIES * nr].reshape(HAMMING_RING_QUERIES, nr)
        for i in range(HAMMING_RING_QUERIES):
            q = np.floor(rng.uniform([70, 70], [cols - 70, rows - 70]) * 2) / 2
            qxy[b, i] = q
            for rank, j in enumerate(rng.permutation(nr)):
                txy[b, slots[i, j]] = q + HAMMING_RING_OFFSETS[j]
                bits = np.zeros(256, np.uint8)
                bits[rng.permutation(256)[:3 * (rank + 1)]] = 1
                td[b, slots[i, j]] = qd[b, i] ^ np.packbits(bits)
    tf = (rng.uniform(0, 1, (B, N)) < 0.05).astype(np.uint8)
    return qd, qxy, td, txy, tf


# -- the chunked bin scan
HAMMING_CHUNKED_ROW = (1022, 1023, 1024, 2160)        # nbins + 1 = 1024 (the last size of the one-entry arm), 1025, 1026, 2162
HAMMING_CHUNKED_GRID = ((1200, 4096, 625.0), (1000, 2600, 625.0), (1000, 2600, 2500.0), (1200, 4096, 5625.0))    # rows, cols, r2: 7 873 and 4 161 entries


@functools.lru_cache(maxsize=2)
def hamming_chunked_row_case(rows):
    """row mode on an image of `rows` rows: 1 200 features over all rows 0 .. rows (every scan chunk populated; the first row, the last, and row `rows`
    itself, which end_y may reach), 500 queries, 30 at either border.  Problem 0 keeps integer rows (the lean walk) and no flag, problem 1 has fractional
    rows and a tenth of its features flagged."""
    B, M, N = 2, 500, 1200
    cols = 3840 if rows > 2000 else 1241
    rng = np.random.default_rng(rows)
    td = rng.integers(0, 256, (B, N, 32), dtype=np.uint8)
    qd = rng.integers(0, 256, (B, M, 32), dtype=np.uint8)
    txy = np.floor(rng.uniform(0, 1, (B, N, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    qxy = (rng.uniform(0, 1, (B, M, 2)) * [cols - 1, rows]).astype(np.float32)
    for b in range(B):
        ys = np.concatenate([np.floor(np.arange(N - 6) * (rows + 1) / (N - 6)), [0, 0, rows, rows, rows - 1, 1]])
        txy[b, :, 1] = rng.permutation(ys).astype(np.float32)
        qxy[b, :30, 1] = rng.uniform(0, 4, 30).astype(np.float32)
        qxy[b, 30:60, 1] = rng.uniform(rows - 4, rows + 3, 30).astype(np.float32)
    txy[1, ::7, 1] += rng.uniform(0.01, 0.99, len(txy[1, ::7])).astype(np.float32)
    tf = (rng.uniform(0, 1, (B, N)) < 0.1).astype(np.uint8)
    tf[0] = 0                                              # (problem 0: every chunk keeps its feature)
    return qd, qxy, td, txy, tf, cols


@functools.lru_cache(maxsize=2)
def hamming_chunked_grid_case(rows, cols):
    """radius mode on a grid of more than 1 023 hash cells: one feature in every chunk of the scan (at a different place of the chunk from chunk to chunk),
    more along the last cell column, the last cell row and the first column (a window at the end of a cell row must not run into the next row's first
    cells); queries beside features and across all four image borders.  Sparse: about 1 400 features."""
    nbx, nby = hamming_grid(0, rows, cols)
    nbins = nbx * nby
    chunk = hamming_scan_chunk(nbins)
    assert chunk > 1 and (nbins + 1) % chunk != 0
    B, M = 2, 700
    rng = np.random.default_rng([rows, cols])
    out_t, out_q = [], []
    for b in range(B):
        c = np.arange(-(-(nbins + 1) // chunk))
        bins = np.minimum(c * chunk + (c + b) % chunk, nbins - 1)
        pts = np.column_stack([bins % nbx, bins // nbx]) * 25.0 + rng.uniform(0.5, 24.5, (len(bins), 2))
        extra = [np.column_stack([rng.uniform(cols - 30, cols - 0.5, 150), rng.uniform(0, rows - 1, 150)]),
                 np.column_stack([rng.uniform(0, cols - 1, 100), rng.uniform(rows - 30, rows - 0.5, 100)]),
                 np.column_stack([rng.uniform(0, 30, 100), rng.uniform(0, rows - 1, 100)]),
                 rng.uniform(0, 1, (50, 2)) * [cols - 1, rows - 1]]
        t = np.vstack([pts] + extra)
        t = np.minimum(t, [cols - 0.25, rows - 0.25])
        t = t[rng.permutation(len(t))]
        near = t[rng.integers(0, len(t), 300)] + rng.uniform(-20, 20, (300, 2))
        q = np.vstack([near,
                       np.column_stack([rng.uniform(cols - 40, cols + 30, 100), rng.uniform(-10, rows + 10, 100)]),
                       np.column_stack([rng.uniform(-10, cols + 10, 100), rng.uniform(rows - 40, rows + 30, 100)]),
                       np.column_stack([rng.uniform(-30, 40, 100), rng.uniform(-10, rows + 10, 100)]),
                       rng.uniform(0, 1, (100, 2)) * [cols - 1, rows - 1]])
        out_t.append(t.astype(np.float32))
        out_q.append(q.astype(np.float32))
    txy, qxy = np.stack(out_t), np.stack(out_q)
    N = txy.shape[1]
    td = rng.integers(0, 256, (B, N, 32), dtype=np.uint8)
    qd = rng.integers(0, 256, (B, M, 32), dtype=np.uint8)
    tf = (rng.uniform(0, 1, (B, N)) < 0.1).astype(np.uint8)
    return qd, qxy, td, txy, tf


# -- range starts of exactly 2048 in the packed family (N = 2048, no feature flagged)
HAMMING_PACKED_LAYOUTS = ("behind", "tail", "control")


@functools.lru_cache(maxsize=3)
def hamming_packed_starts_case(layout):
    """N = 2048 unflagged features on 1241 x 376 (50 x 16 cells), r2 = 625, M = 300, B = 2.
    behind : every feature in cell rows 0 .. 3; 100 queries from cell row 6 down (all three range starts are 2048), 100 in cell rows 4 and 5 (the first
             window row may still hold features), 100 among the features
    tail   : cell rows 0 .. 4 full, and the last features in bin order in cells (5, 10 .. 12): 2 + 2 + 2 in problem 0 (even counts), 2 + 2 + 3 in problem 1
             (odd); 100 queries in cell row 6 above them -- their first range ends at feature 2048, the two behind it start there -- the rest anywhere
    control: `tail` with N = 2047"""
    rows, cols = HAMMING_GEOMETRY
    B, M = 2, 300
    N = 2047 if layout == "control" else 2048
    rng = np.random.default_rng(["behind", "tail", "control"].index(layout) + 2048)
    td = rng.integers(0, 256, (B, N, 32), dtype=np.uint8)
    qd = rng.integers(0, 256, (B, M, 32), dtype=np.uint8)
    txy = np.empty((B, N, 2), np.float32)
    qxy = (rng.uniform(0, 1, (B, M, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    for b in range(B):
        if layout == "behind":
            txy[b] = rng.uniform([0, 0], [cols - 1, 99.5], (N, 2))
            qxy[b, :100] = rng.uniform([0, 150], [cols - 1, rows + 20], (100, 2))
            qxy[b, 100:200] = rng.uniform([0, 100], [cols - 1, 149.5], (100, 2))
            qxy[b, 200:] = rng.uniform([0, 0], [cols - 1, 99.5], (100, 2))
        else:
            tail = [2, 2, 2 + b]
            n_tail = sum(tail)
            txy[b, :N - n_tail] = rng.uniform([0, 0], [cols - 1, 124.5], (N - n_tail, 2))
            cells = np.repeat([10, 11, 12], tail)
            txy[b, N - n_tail:] = np.column_stack([cells * 25 + rng.uniform(1, 24, n_tail), rng.uniform(140, 149.5, n_tail)])
            txy[b] = txy[b, rng.permutation(N)]
            qxy[b, :100] = np.column_stack([rng.uniform(265, 349, 100), rng.uniform(150, 174.5, 100)])
    return qd, qxy, td, txy, np.zeros((B, N), np.uint8)


# -- the constructed input of the 11-bit overflow: a phantom candidate that IS inside a circle
def hamming_phantom_case():
    """N = 2048 unflagged features, M = 1099, r2 = 625 on 1241 x 376: built so that the start fields' overflow, unguarded, changes a record.
    Every feature lies in cell rows 0 .. 3 but two, in cell (4, 1).  Query Q = (3, 128) (the last but ten) has those two as its first range -- an even
    length that ends at feature 2048 -- and nothing behind: starts 2048, 2048.  Packed into 11-bit fields the first of them turns length 2 into 3, and
    the third candidate is LDS position 2048: s_xy[N], the slot words of query 0 read as coordinates (x, y).
      x: word 0 = s0 | s1 << 11 | l0 << 22, a float with exponent field l0 >> 1 <= 31: below 1e-28, whatever query 0 is.
      y: word 1 = s2 | l1 << 11 | l2 << 17 | hi << 23 once stage 4a has stored query 0's mask: exponent field = bits 32 .. 39 of the in-circle mask.
    Query 0 = (262.5, 37.5) sees 40 window candidates in cell order (0,9) (0,10) (0,11) | (1,9) (1,10) (1,11) | (2,10): 20 | 13 outside its circle, 2
    inside, 4 outside | 1 inside.  Candidates 32 .. 39 are out, in, in, out x 4, in whatever order each cell's features took: hi = 0b10000110 = 134,
    y = 2^7 (1 + (19 << 11 | 1 << 17) / 2^23) = 130.6, inside Q's circle, where the reference has no candidate at all.
    For Q to read the word AFTER query 0's mask is stored: 960 queries with 60 or more window candidates each (matched in place in stage 4a) fill the
    first fifteen wavefronts of round 0, query 0 leads the sixteenth, followed by 127 queries of 30 candidates; Q is the 1089th in sorted order and
    falls to round 1 of a wavefront that spent round 0 on descriptor walks.  (No barrier orders the two: the unguarded kernel gives the wrong record
    when the wavefronts run as described, the right one otherwise.)
    Returns (qd, qxy, td, txy, tf, info)."""
    rows, cols = HAMMING_GEOMETRY
    nbx, nby = hamming_grid(0, rows, cols)
    rng = np.random.default_rng(134)
    q0 = np.array([262.5, 37.5])
    in_cell = lambda cy, cx, n: np.column_stack([cx * 25 + rng.uniform(1, 24, n), cy * 25 + rng.uniform(1, 24, n)])
    feats = {}                                                     # (cy, cx) -> points
    feats[(0, 9)], feats[(0, 10)], feats[(0, 11)] = in_cell(0, 9, 7), in_cell(0, 10, 7), in_cell(0, 11, 6)
    feats[(1, 9)] = np.column_stack([rng.uniform(226, 236, 13), rng.uniform(26, 49, 13)])
    feats[(1, 10)] = np.array([[262.0, 38.0], [263.0, 37.0]])
    feats[(1, 11)] = np.column_stack([rng.uniform(290, 299, 4), rng.uniform(26, 49, 4)])
    feats[(2, 10)] = np.array([[262.0, 52.0]])
    feats[(2, 9)] = feats[(2, 11)] = np.zeros((0, 2))
    spot2 = [(cy, cx) for cy in (0, 1, 2) for cx in (29, 30, 31)]
    for (cy, cx), n in zip(spot2, (4, 3, 3, 4, 3, 3, 4, 3, 3)):
        feats[(cy, cx)] = in_cell(cy, cx, n)
    feats[(4, 1)] = np.array([[45.0, 101.0], [46.0, 102.0]])
    dense = [(cy, cx) for cy in range(4) for cx in range(nbx) if (cy, cx) not in feats]
    left = 2048 - sum(len(v) for v in feats.values())
    base, more = divmod(left, len(dense))
    for i, (cy, cx) in enumerate(dense):
        feats[(cy, cx)] = in_cell(cy, cx, base + (i < more))
    txy = np.vstack([feats[k] for k in sorted(feats)])
    assert len(txy) == 2048
    txy = txy[rng.permutation(2048)].astype(np.float32)
    heavy_cols = [c for c in range(3, 47) if min(abs(c - 10), abs(c - 30)) > 3]
    heavy = np.column_stack([rng.choice(heavy_cols, 960) * 25 + rng.uniform(1, 24, 960), rng.uniform(1, 74, 960)])
    medium = np.column_stack([30 * 25 + rng.uniform(1, 24, 127), 25 + rng.uniform(1, 24, 127)])
    Q = np.array([[3.0, 128.0]])
    light = np.column_stack([rng.uniform(0, cols - 1, 10), rng.uniform(210, rows - 1, 10)])
    qxy = np.vstack([q0[None], heavy, medium, Q, light]).astype(np.float32)
    M = len(qxy)
    td = rng.integers(0, 256, (2048, 32), dtype=np.uint8)
    qd = rng.integers(0, 256, (M, 32), dtype=np.uint8)
    info = dict(q0=0, heavy=np.arange(1, 961), medium=np.arange(961, 1088), Q=1088, light=np.arange(1089, M))
    return qd[None], qxy[None], td[None], txy[None], np.zeros((1, 2048), np.uint8), info


def hamming_packed_words(qxy, txy, rows, cols):
    """the packed family's slot words of every query as stage 3 would store them WITHOUT a guard on the starts (N <= 2048, no flags), and the ranges:
    (W0, W1, s (M, 3), l (M, 3)); W0 = 0xFFFFFFFF where a length reaches 64.  Bin order is (cell row, cell column); starts are counts of features in
    earlier bins."""
    nbx, nby = hamming_grid(0, rows, cols)
    cell = lambda v: np.floor(v.astype(np.float32) / np.float32(HASH_CELL)).astype(np.int64)
    tb = np.clip(cell(txy[:, 1]), 0, nby - 1) * nbx + np.clip(cell(txy[:, 0]), 0, nbx - 1)
    start = np.concatenate([[0], np.cumsum(np.bincount(tb, minlength=nbx * nby))])
    hx, hy = cell(qxy[:, 0]), cell(qxy[:, 1])
    x0, x1 = np.maximum(hx - 1, 0), np.minimum(hx + 1, nbx - 1)
    y0, y1 = np.maximum(hy - 1, 0), np.minimum(hy + 1, nby - 1)
    s, l = np.zeros((len(qxy), 3), np.int64), np.zeros((len(qxy), 3), np.int64)
    for k in range(3):
        ok = (y0 + k <= y1) & (x0 <= x1)
        row = np.where(ok, (y0 + k) * nbx, 0)
        s[:, k] = start[row + np.where(ok, x0, 0)]
        l[:, k] = start[row + np.where(ok, x1 + 1, 0)] - s[:, k]
    fits = (l < 64).all(axis=1)
    W0 = np.where(fits, (s[:, 0] | (s[:, 1] << 11) | (l[:, 0] << 22)) & 0xFFFFFFFF, 0xFFFFFFFF).astype(np.uint32)
    W1 = ((s[:, 2] | (l[:, 1] << 11) | (l[:, 2] << 17)) & 0xFFFFFFFF).astype(np.uint32)
    return W0, W1, s, l


def hamming_count_check(csr):
    """asserts that every query of hamming_count_case(csr) sees its population's counts range by range, and that about half of them lie inside the
    circle; returns [(k, layout, longest range, features at distance^2 == r2 from the cell's centre)]"""
    from hamming_util import radius_mask
    rows, cols = HAMMING_COUNT_GEOMETRY
    qd, qxy, td, txy, tf, pops = hamming_count_case(csr)
    r2 = np.float32(625.0 * csr * csr)
    stats = []
    for b in range(2):
        assert not tf[b].any()
        wc = hamming_window_counts(qxy[b], txy[b], tf[b], csr, rows, cols)
        inside = radius_mask(qxy[b], txy[b], r2)
        for k, layout, per, qi in pops:
            want = [per.get(j, 0) for j in range(-csr, csr + 1)]
            assert sum(want) == k and (wc[qi] == want).all(), (csr, b, k, layout)
            n_in = inside[qi].sum(axis=1)
            assert (n_in >= k // 4).all() and (n_in <= k - k // 4).all(), (csr, b, k, layout, n_in.min(), n_in.max())
            main = qi[::4][0]
            d = txy[b] - qxy[b, main]
            n_exact = int(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float32) == r2).sum())
            if b == 0:
                stats.append((k, layout, max(want), n_exact))
    return stats


# ---- BRIEF at every seam of `inside`, both kernels (test_gpu_brief_seams.py) ---------------------------------------------------------------------------
# brief_border_keep keeps a corner whose ROUNDED-TO-EVEN position lies in [28, W - 28) x [28, H - 28); BRIEF samples around (int)(x + 0.5), (int)(y + 0.5).
# The two differ at .5 ties, so the centre (cx, cy) of a kept corner reaches [28, W - 28] x [28, H - 28].  k_brief's 49 x 49 window (radius 24) is inside the
# image for all of them; k_brief_img's 57 x 57 patch (radius 28, fetched as 64 columns from the word boundary at or left of cx - 28) is not:
#   bottom    cy = H - 28 (y = H - 28.5 with H odd: H - 29 is even, the tie rounds down and the corner is kept): cy + 28 < H fails
#   overrun   ((cx - 28) & ~3) + 64 <= pitch fails for cx > W - 33 where the row pitch equals W, i.e. W a multiple of 64: the four last kept columns
# and such a corner takes the clipped element-wise path.  128 x 97 is the smallest image with W a multiple of 64 that holds the column list W - 40 .. W - 28.
BRIEF_SEAM_W, BRIEF_SEAM_H, BRIEF_SEAM_DISP, BRIEF_SEAM_FRAMES = 128, 97, 4, 3
BRIEF_BORDER = 28


def brief_seam_corners(W=BRIEF_SEAM_W, H=BRIEF_SEAM_H):
    """the left eye's corner list (float64, (x, y)): every integer column W - 40 .. W - 28 at two rows; .5 ties and their neighbours on all four borders;
    interior corners at eight consecutive columns (both parities of cx - 24, all four values of (cx - 28) & 3), whole and fractional"""
    c = [(float(x), y) for y in (33.0, 60.0) for x in range(W - 40, W - 27)]
    c += [(x, 45.0 + k) for k, x in enumerate((26.5, 27.5, 28.0, 28.25, 28.5, W - 29.5, W - 29.25, W - 29.0, W - 28.5, W - 27.5))]
    c += [(44.0 + 3 * k, y) for k, y in enumerate((26.5, 27.5, 28.0, 28.25, 28.5, H - 29.5, H - 29.25, H - 29.0, H - 27.5))]
    c += [(x, H - 28.5) for x in (36.0, 52.5, 71.0, W - 30.0)]                 # cy = H - 28: below every kept integer row
    c += [(40.0 + k, 50.0) for k in range(8)] + [(40.3 + k, 39.6) for k in range(8)]
    return np.array(c, dtype=np.float64)


def brief_seam_expected(corners, W=BRIEF_SEAM_W, H=BRIEF_SEAM_H):
    """(kept mask, cx, cy) of a corner list by the two rules restated in numpy: float32 coordinates, rint (half to even) for the filter, (int)(v + 0.5) in
    double for the centre"""
    xy = corners.astype(np.float32)
    r = np.rint(xy).astype(np.int64)
    keep = (r[:, 0] >= BRIEF_BORDER) & (r[:, 0] < W - BRIEF_BORDER) & (r[:, 1] >= BRIEF_BORDER) & (r[:, 1] < H - BRIEF_BORDER)
    c = np.floor(xy.astype(np.float64) + 0.5).astype(np.int64)
    return keep, c[:, 0], c[:, 1]


def brief_seam_tally(corners, W=BRIEF_SEAM_W, H=BRIEF_SEAM_H):
    """kept corners per seam: on the last centre that is inside (left, top, right, bottom) and on the two conditions that fail for k_brief_img"""
    keep, cx, cy = brief_seam_expected(corners, W, H)
    cx, cy = cx[keep], cy[keep]
    pitch = (W + 63) // 64 * 64
    overrun = ((cx - 28) & ~3) + 64 > pitch
    return dict(kept=int(keep.sum()), left=int((cx == 28).sum()), top=int((cy == 28).sum()), right=int((cx == W - 29).sum()),
                bottom=int((cy == H - 29).sum()), below=int((cy == H - 28).sum()), overrun=int(overrun.sum()),
                slow_img=int((overrun | (cy + 28 >= H) | (cx + 28 >= W)).sum()),
                slow_plane=int(((cx - 24 < 0) | (cx + 24 >= W) | (cy - 24 < 0) | (cy + 24 >= H)).sum()),
                parity=sorted(set(((cx - 24) & 1).tolist())), quarter=sorted(set(((cx - 28) & 3)[~overrun].tolist())))


def brief_seam_case():
    """(params, [(L, R, corners_left, corners_right)]): one noise pair (the right eye is the left one moved BRIEF_SEAM_DISP px), the seam list in the left
    eye and its partners in the right one, the same frame BRIEF_SEAM_FRAMES times: a static camera that keeps tracking on its own map"""
    W, H = BRIEF_SEAM_W, BRIEF_SEAM_H
    prm = lvt_amd.kitti_params(width=W, height=H)
    L = np.random.default_rng(40).integers(0, 256, (H, W), dtype=np.uint8)
    R = np.ascontiguousarray(np.roll(L, -BRIEF_SEAM_DISP, axis=1))
    cl = brief_seam_corners(W, H)
    cr = cl - [[float(BRIEF_SEAM_DISP), 0.0]]
    return prm, [(L, R, cl, cr)] * BRIEF_SEAM_FRAMES


# ---- bookkeeping across the 1024-point seam, and LOST on a large map (test_gpu_map_capacity.py) -----------------------------------------------------
# k_track_mid sends a map of up to RES_THREADS = 1024 points through bookkeep_cull_small and a larger one through bookkeep_cull_large.  The recipes above
# run the large body at 10 k points and more, the parity sequences the small one at ~800.  Two more, of the same construction (a fixed strip of MAPCAP_KEEP
# corners that every frame matches, fresh corners per texture epoch that triangulate once and are never seen again):
#   seam   fresh corners per frame chosen so that the map at match time climbs through (896, 1024] into (1024, 1152], is culled back below 1024 and climbs again
#   lost   a map of more than 1024 points, then a frame without the fixed strip's texture: fewer than min_num_matches matches -> LOST.  The large body applies
#          its bookkeeping IN PLACE then (no compaction, the map buffer is not swapped): counters and ages of all points are what map() shows afterwards
# name: (overrides, fresh corners per frame; None = the LOST frame)
MAPSEAM_RECIPES = {
    "seam": ({"staged_threshold": 0, "untracked_threshold": 2}, (640, 130, 130, 130, 700, 130, 130)),
    "lost": ({"staged_threshold": 0, "untracked_threshold": 1000, "min_num_matches_for_tracking": 100}, (640, 300, 300, None, 300)),
}


def mapseam_case(name):
    """(params, [(L, R, corners_left, corners_right)]): mapcap_frame's construction with the recipe's number of fresh corners per frame.  The LOST frame is a
    fresh noise pair (nothing of the fixed strip) with forty corners"""
    overrides, fresh = MAPSEAM_RECIPES[name]
    prm = lvt_amd.kitti_params(width=MAPCAP_W, height=MAPCAP_H)
    prm.triangulation_policy = 2
    for k, v in overrides.items():
        setattr(prm, k, type(getattr(prm, k))(v))
    fixed, keep = _mapcap_fixed()
    frames = []
    for i, n in enumerate(fresh):
        rng = np.random.default_rng(300 + i)
        L = rng.integers(0, 256, (MAPCAP_H, MAPCAP_W), dtype=np.uint8)
        if n is not None:
            L[:, :300] = fixed[:, :300]
        R = np.ascontiguousarray(np.roll(L, -MAPCAP_DISP, axis=1))
        pts = np.column_stack([rng.integers(340, MAPCAP_W - 40, n or 40), rng.integers(40, MAPCAP_H - 40, n or 40)])
        cl = np.unique(np.vstack([keep, pts]) if n is not None else pts, axis=0).astype(np.float64)
        frames.append((L, R, cl, cl - [[float(MAPCAP_DISP), 0.0]]))
    return prm, frames
