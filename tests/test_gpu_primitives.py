"""-m gpu: stage-level differential tests of individual kernels against the oracle's primitives."""
import numpy as np
import pytest

from case_tables import (PNP_EDGE_COUNTS, PNP_HARD, PNP_HARD_UNSTAGED, PNP_INTRINSICS, PNP_STAGE_MAX, pnp_case as _pnp_case,
                         pnp_edge_case, pnp_hard_case as _pnp_hard_case, pnp_prior_cases, trace_noise)
from hamming_util import NO_NEIGHBOUR, problem_mask

pytestmark = pytest.mark.gpu


def _plane_expected(O, img, prm):
    H, W = img.shape
    cs = prm.detection_cell_size
    t_low = int(prm.agast_threshold * 0.5 + 0.5)
    out = np.zeros((H, W), np.int32)
    for y0 in range(0, H, cs):
        for x0 in range(0, W, cs):
            sm = O.agast_score_map(np.ascontiguousarray(img[y0:y0 + cs, x0:x0 + cs])).astype(np.int32)
            sm[sm < t_low] = 0
            out[y0:y0 + cs, x0:x0 + cs] = sm
    return out


FEATURE_GEOMETRY = [
    # id, image size, world seed, cell size, key points per cell (None: KITTI's shape, cell 250, 150 key points; noise fills every cell: at most
    # NF_MAX = 4 096 features per image)
    ("kitti", None, 11, None, None),
    ("cells_48", (620, 188), 32, 48, 30),         # below one k_score tile: pass 0 compacts the score map, a tile holds two cell boundaries
    ("cells_64", (620, 188), 32, 64, 100),        # smallest size with k_score's segments
    ("cells_100", (1241, 376), 33, 100, 40),      # 52 cells, 41-px last column, 76-row last row
    ("cells_257", (1241, 376), 33, 257, 150),     # row strips + three-launch ANMS on cells other than 0 too
    ("cells_1024", (1241, 376), 33, 1024, 600),   # the widest cell on the LDS paths
    ("cells_2000", (1241, 376), 33, 2000, 1000),  # one 1241 x 376 cell: the wide global path
    ("one_interior_px", (757, 507), 34, 250, 150),
    ("no_interior", (753, 506), 34, 250, 150),
]
# cell 0's route through k_cells_big (debug_stamps()[10]): 1001 / 1002 strips, 1003 the whole cell on global scratch; 1004 the wide global path
ROUTES = {("cells_257", "noise"): (1001, 1002), ("cells_257", "noise_tall_blob"): (1003,), ("cells_1024", "world"): (1001, 1002),
          ("cells_1024", "noise"): (1003,), ("cells_2000", "world"): (1004,), ("cells_2000", "noise"): (1004,)}
_GEO_CASES = [(g, k) for g in FEATURE_GEOMETRY for k in ("noise", "world")] + [(FEATURE_GEOMETRY[4], "noise_tall_blob")]


@pytest.mark.parametrize("geo,kind", _GEO_CASES, ids=[k if g[1] is None else f"{g[0]}-{k}" for g, k in _GEO_CASES])
def test_score_and_boxsum_planes(hip_lib, oracle_lib, geo, kind):
    """k_score: per-cell OAST-9/16 score (incl. the 3-px dead band of every cell) and the 9x9 box sums, every pixel, and both images' features --
    key points, responses, descriptors, order -- against the oracle; on KITTI's shape and on the shapes where the feature stage changes its route"""
    from parity_util import make_case
    from oracle import pyoracle
    name, size, seed, cs, max_kp = geo
    overrides = {} if cs is None else {"detection_cell_size": cs, "max_keypoints_per_cell": max_kp}
    world, prm, _ = make_case("kitti", seed, 1.0, overrides, size=size)
    H, W = world.H, world.W
    rng = np.random.default_rng(0 if cs is None else cs)
    if kind == "noise":      # corner-dense worst case: the stress for NMS + ANMS + the std::sort emulation
        L = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
        R = np.ascontiguousarray(L[:, ::-1])
    elif kind == "noise_tall_blob":   # enough raw corners for the strips, and a 4-connected corner blob 137 rows tall across them: they cannot vouch
        L = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
        L[50:210, 80:120] = 20
        L[60:200, 96:101] = np.tile(np.array([[128, 128, 128, 128, 20], [128, 235, 128, 235, 128]], np.uint8), (70, 1))
        R = np.ascontiguousarray(L[:, ::-1])
    else:
        L, R = world.render_stereo(0)
    hip = hip_lib.LvtSystem.create(prm, 1)
    hip.track(L, R)
    for eye, img in ((0, L), (1, R)):
        sp = hip.plane(eye, 0)[:, :W].astype(np.int32)
        assert np.array_equal(sp, _plane_expected(oracle_lib, img, prm)), f"score plane eye {eye}"
        a = np.pad(img.astype(np.int64), 4)
        box = sum(a[dy:dy + H, dx:dx + W] for dy in range(9) for dx in range(9))
        assert np.array_equal(hip.plane(eye, 1)[:, :W].astype(np.int64), box), f"box sums eye {eye}"
        xo, ro, do, _ = pyoracle.compute_features(img, prm)
        xh, rh, dh = hip.features(eye)
        assert len(xo) > 0
        assert np.array_equal(xh, xo) and np.array_equal(rh, ro) and np.array_equal(dh, do), (name, kind, eye, len(xh), len(xo))
    if (name, kind) in ROUTES:
        assert int(hip.debug_stamps()[10]) in ROUTES[(name, kind)], (name, kind, int(hip.debug_stamps()[10]))
    assert hip.counts()["overflow"] == 0, hip.counts()["overflow"]
    # (only noise on a whole-cell path may outlast the early stream's gate waits: reported, results unaffected)
    err = hip.last_error()
    assert err == "" or (kind.startswith("noise") and "results unaffected" in err), err


def test_anms_decision_across_the_largest_cell(hip_lib, oracle_lib):
    """one 4096 x 1200 detection cell -- CELL_SIDE_MAX wide, the wide global path -- whose ANMS decision radius is a distance of about 4 100 px:
    radius^2 over 2^24, past three 8-bit digits of the radix select.  A strong square top left, a weaker one bottom right (its corners' only
    1.11x-stronger neighbours are the first square's), weaker squares 1 000 px apart between them; six key points per cell put the decision on
    the bottom-right square's corners.  Key points, responses, descriptors and order against the oracle."""
    from oracle import pyoracle
    W, H = 4096, 1200
    prm = hip_lib.tum_params(width=W, height=H, fx=2000.0, fy=2000.0, cx=W / 2.0, cy=H / 2.0)
    prm.detection_cell_size = 5000
    prm.max_keypoints_per_cell = 6
    img = np.full((H, W), 100, np.uint8)
    img[40:52, 40:52] = 255
    img[1130:1142, 4030:4042] = 200
    for k, v in enumerate((180, 165, 152)):                               # each more than 1.11x weaker than the one before
        img[500:512, 1000 * (k + 1):1000 * (k + 1) + 12] = v
    hip = hip_lib.LvtSystem.create(prm, 2)
    hip.track(img, np.full((H, W), 2.0, np.float32))
    xo, ro, do, _ = pyoracle.compute_features(img, prm)
    xh, rh, dh = hip.features(0)
    assert len(xo) >= 6 and xo[:, 0].max() > 4000 and xo[:, 0].min() < 100, xo
    assert np.array_equal(xh, xo) and np.array_equal(rh, ro) and np.array_equal(dh, do), (xh, xo)
    assert int(hip.debug_stamps()[10]) == 1004
    assert hip.counts()["overflow"] == 0 and hip.last_error() == "", hip.last_error()


@pytest.mark.parametrize("kind", ["noise", "blurred_noise", "tall_blobs", "world"])
def test_oversized_cell_paths(hip_lib, oracle_lib, kind):
    """the RGB-D configuration's single 640x480 detection cell on inputs that push it through every route: uniform noise (every strip
    overflows its LDS: whole-cell path on global scratch), blurred noise, an ordinary frame (strips + three-launch ANMS) and noise
    stretched vertically (corner blobs taller than a strip's halo: the strips cannot vouch, whole-cell path again) -- key points, responses,
    descriptors and their ORDER against the oracle"""
    from parity_util import make_case
    from oracle import pyoracle
    world, prm, _ = make_case("tum", 4, 1.0)
    H, W = world.H, world.W
    rng = np.random.default_rng(7)
    if kind == "noise":
        img = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    elif kind == "world":
        img = world.render_rgbd(0)[0]                                         # an ordinary frame: strips + three-launch ANMS
    elif kind == "blurred_noise":
        a = rng.integers(0, 256, size=(H + 2, W + 2)).astype(np.float32)
        img = ((a[:-2, :-2] + a[:-2, 1:-1] + a[:-2, 2:] + a[1:-1, :-2] + a[1:-1, 1:-1] + a[1:-1, 2:] + a[2:, :-2] + a[2:, 1:-1] + a[2:, 2:]) / 9.0)
        img = np.clip((img - 128.0) * 3.0 + 128.0, 0, 255).astype(np.uint8)
    else:
        a = rng.integers(0, 256, size=(H + 23, W)).astype(np.float32)
        c = np.cumsum(np.vstack([np.zeros((1, W), np.float32), a]), axis=0)
        img = (c[24:] - c[:-24]) / 24.0                                        # 24-row vertical box blur: structures (and corner blobs) stretched along y
        img = np.clip((img - 128.0) * 6.0 + 128.0, 0, 255).astype(np.uint8)[:H]
        img = np.ascontiguousarray(img)
    depth = np.full((H, W), 2.0, np.float32)
    hip = hip_lib.LvtSystem.create(prm, 2)
    hip.track(img, depth)
    xo, ro, do, _ = pyoracle.compute_features(img, prm)
    xh, rh, dh = hip.features(0)
    assert len(xo) > 0 or kind == "tall_blobs"
    assert np.array_equal(xh, xo) and np.array_equal(rh, ro) and np.array_equal(dh, do), (kind, len(xh), len(xo))
    route = int(hip.debug_stamps()[10])   # written by k_cells_big: 1001 strips + three-launch ANMS, 1002 strips without ANMS, 1003 whole-cell path
    assert route in {"noise": (1003,), "blurred_noise": (1001, 1002, 1003), "tall_blobs": (1003,), "world": (1001,)}[kind], (kind, route, len(xo))
    # (the whole-cell path on 300 000 noise pixels takes longer than the early stream's 20-ms gate waits: reported, results unaffected)
    err = hip.last_error()
    assert err == "" or "results unaffected" in err, err


# (LVT_AMD_CELL_SPLIT, input): None = the default of two strips.  The strip arithmetic (strip_nms) is shared by 2, 3 and -- the oversized cells -- 8 strips
_SPLIT_CASES = [(None, "world"), (None, "tall_blobs"), (None, "blurred_noise"), ("3", "world"), ("3", "tall_blobs"), ("0", "world")]


@pytest.mark.parametrize("split,kind", _SPLIT_CASES, ids=[k if s is None else f"split{s}-{k}" for s, k in _SPLIT_CASES])
def test_split_cell_routes(hip_lib, oracle_lib, monkeypatch, split, kind):
    """a single sequence's 250-row detection cells run as TWO co-operating workgroups of one k_cells launch (cells_work_split: AGAST's NMS of the
    upper and the lower half with a 16-row halo, survivors merged, ANMS on the merged list).  An ordinary frame takes the split; noise stretched
    a constructed corner blob 137 rows tall crosses the cut and both halos -- the strips cannot vouch and the main workgroup runs the whole cell alone (route 2003).
    Key points, responses, descriptors and their ORDER against the oracle either way.
    LVT_AMD_CELL_SPLIT=3: three strips -- the middle one's core rows are [85, 167) of the 250-row cell and its extended rows [69, 183); the planted blob (rows
    60 - 200) touches both outer rows and the core, so that strip cannot vouch either.  =0: no split, the whole cell on one workgroup from the start."""
    from parity_util import make_case
    from oracle import pyoracle
    if split is not None:
        monkeypatch.setenv("LVT_AMD_CELL_SPLIT", split)   # (read when the handle is created)
    world, prm, _ = make_case("kitti", 4, 1.0)
    H, W = world.H, world.W
    rng = np.random.default_rng(11)
    if kind == "world":
        img = world.render_stereo(0)[0]
    elif kind == "blurred_noise":
        a = rng.integers(0, 256, size=(H + 2, W + 2)).astype(np.float32)
        img = ((a[:-2, :-2] + a[:-2, 1:-1] + a[:-2, 2:] + a[1:-1, :-2] + a[1:-1, 1:-1] + a[1:-1, 2:] + a[2:, :-2] + a[2:, 1:-1] + a[2:, 2:]) / 9.0)
        img = np.clip((img - 128.0) * 3.0 + 128.0, 0, 255).astype(np.uint8)
    else:
        # a 5 x 2 tile repeated down a column makes EVERY pixel of one image column a corner (found by search over small tiles with the oracle's score
        # map): a 4-connected corner blob 137 rows tall in cell 0 -- through the cut between the two strips and both their halos
        img = world.render_stereo(0)[0].copy()
        img[50:210, 80:120] = 20
        img[60:200, 96:101] = np.tile(np.array([[128, 128, 128, 128, 20], [128, 235, 128, 235, 128]], np.uint8), (70, 1))
    img = np.ascontiguousarray(img)
    hip = hip_lib.LvtSystem.create(prm, 1)
    hip.track(img, img)
    xo, ro, do, _ = pyoracle.compute_features(img, prm)
    xh, rh, dh = hip.features(0)
    assert np.array_equal(xh, xo) and np.array_equal(rh, ro) and np.array_equal(dh, do), (kind, len(xh), len(xo))
    route = int(hip.debug_stamps()[10])
    if kind == "world":
        assert route != 2003 and len(xo) > 500, (route, len(xo))
    if kind == "tall_blobs":
        assert route == 2003, (route, len(xo))
    assert hip.last_error() == "", hip.last_error()


def _hamming_ref(O, qd, qxy, td, txy, tf, r2, mode, rows, cols):
    B, M = qd.shape[:2]
    out = np.zeros((B, M, 4), np.int32)
    for b in range(B):
        mask = problem_mask(qxy[b], txy[b], tf[b], r2, mode, rows).astype(np.uint8)
        for m in range(M):
            out[b, m] = O.hamming_top2(qd[b, m], td[b], mask[m])
    return out


@pytest.mark.parametrize("mode,variant", [(0, "random"), (0, "ties"), (0, "planted"), (0, "all_masked"), (1, "random"), (1, "ties")])
def test_hamming_match_batched(hip_lib, oracle_lib, mode, variant):
    """k_hamming_batched vs cv::BFMatcher knnMatch(k=2, mask) semantics: top-2, ties -> lowest index"""
    import torch
    rng = np.random.default_rng(42)
    B, M, N, rows, cols = 5, 96, 333, 376, 1241
    td = rng.integers(0, 256, (B, N, 32), dtype=np.uint8)
    qd = rng.integers(0, 256, (B, M, 32), dtype=np.uint8)
    if variant == "ties":          # descriptors drawn from 6 prototypes: massive distance ties
        proto = rng.integers(0, 256, (6, 32), dtype=np.uint8)
        td = proto[rng.integers(0, 6, (B, N))]; qd = proto[rng.integers(0, 6, (B, M))]
    if variant == "planted":
        src = rng.integers(0, N, (B, M))
        qd = np.take_along_axis(td, src[:, :, None], axis=1).copy()
        qd[:, :, 0] ^= 0x11
    txy = np.floor(rng.uniform(0, 1, (B, N, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    if variant == "planted":
        qxy = np.take_along_axis(txy, np.repeat(src[:, :, None], 2, 2), axis=1) + rng.uniform(-3, 3, (B, M, 2)).astype(np.float32)
    else:
        qxy = (rng.uniform(0, 1, (B, M, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    qxy = qxy.astype(np.float32)
    tf = (rng.uniform(0, 1, (B, N)) < 0.2).astype(np.uint8)
    if variant == "all_masked":
        tf[:] = 1
    r2 = 625.0 if variant != "ties" else 2500.0
    ref = _hamming_ref(oracle_lib, qd, qxy, td, txy, tf, r2, mode, rows, cols)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = torch.zeros((B, M, 4), dtype=torch.int32, device="cuda")
    us = hip_lib.hamming_match_batched(t(qd), t(qxy), t(td), t(txy), t(tf), r2, mode, rows, cols, out)
    assert us > 0
    got = out.cpu().numpy()
    assert np.array_equal(got, ref), f"first mismatch {np.argwhere(got != ref)[:3]}"


def _hamming_ref_np(qd, qxy, td, txy, tf, r2, mode, rows):
    """vectorised restatement of the same semantics (masked top-2, ties -> lowest index) for sizes the scalar oracle loop
    would take minutes on; checked against the oracle on the small cases above by construction of the same masks (hamming_util.py, which
    also holds the cheap reference of the sizes this one's (M, N, 32) table cannot reach: test_hamming_reference.py holds the two together)"""
    B, M = qd.shape[:2]
    N = td.shape[1]
    out = np.zeros((B, M, 4), np.int32)
    pop = np.array([bin(i).count("1") for i in range(256)], np.int32)
    for b in range(B):
        d = pop[qd[b][:, None, :] ^ td[b][None, :, :]].sum(axis=2).astype(np.int64)      # (M, N)
        mask = problem_mask(qxy[b], txy[b], tf[b], r2, mode, rows)
        key = np.where(mask, d * 65536 + np.arange(N)[None, :], np.int64(1) << 40)
        key = np.concatenate([key, np.full((M, 2), np.int64(1) << 40)], axis=1)   # (a single train feature still has a "second")
        order = np.argsort(key, axis=1, kind="stable")[:, :2]
        k1 = np.take_along_axis(key, order[:, :1], 1)[:, 0]
        k2 = np.take_along_axis(key, order[:, 1:2], 1)[:, 0]
        big = np.int64(1) << 40
        out[b, :, 0] = np.where(k1 < big, k1 % 65536, NO_NEIGHBOUR[0])
        out[b, :, 1] = np.where(k1 < big, k1 // 65536, NO_NEIGHBOUR[1])
        out[b, :, 2] = np.where(k2 < big, k2 % 65536, NO_NEIGHBOUR[0])
        out[b, :, 3] = np.where(k2 < big, k2 // 65536, NO_NEIGHBOUR[1])
    return out


@pytest.mark.parametrize("mode,r2,M,N", [(0, 625.0, 1100, 1700), (0, 2500.0, 700, 1200), (0, 40000.0, 300, 900), (1, 0.0, 1100, 1700),
                                         (0, 625.0, 2048, 2048), (0, 625.0, 513, 1025)])
def test_hamming_match_batched_large(hip_lib, mode, r2, M, N):
    """every template variant of k_hamming_batched (queries / train features per thread 1..4; 3-, 5- and any-range windows;
    row mode) at sizes where all lanes and both query stages are busy; flags, clustered points (windows > 64 candidates)"""
    import torch
    rng = np.random.default_rng(7 + M + N)
    B, rows, cols = 3, 376, 1241
    td = rng.integers(0, 256, (B, N, 32), dtype=np.uint8)
    qd = rng.integers(0, 256, (B, M, 32), dtype=np.uint8)
    txy = np.floor(rng.uniform(0, 1, (B, N, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    qxy = (rng.uniform(0, 1, (B, M, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    # problem 1: a dense cluster, so that many windows hold more than 64 candidates (one-stage fallback inside stage A)
    txy[1, : N // 2] = np.floor(rng.uniform(0, 1, (N // 2, 2)) * [120, 90] + [300, 100]).astype(np.float32)
    qxy[1, : M // 2] = (rng.uniform(0, 1, (M // 2, 2)) * [120, 90] + [300, 100]).astype(np.float32)
    # problem 2: descriptor ties (8 prototypes) and queries outside the image
    proto = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    td[2] = proto[rng.integers(0, 8, N)]
    qd[2] = proto[rng.integers(0, 8, M)]
    qxy[2, :20] = (rng.uniform(-60, 0, (20, 2))).astype(np.float32)
    qxy[2, 20:40] += np.float32(1300)
    tf = (rng.uniform(0, 1, (B, N)) < 0.15).astype(np.uint8)
    ref = _hamming_ref_np(qd, qxy, td, txy, tf, r2, mode, rows)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = torch.zeros((B, M, 4), dtype=torch.int32, device="cuda")
    us = hip_lib.hamming_match_batched(t(qd), t(qxy), t(td), t(txy), t(tf), r2, mode, rows, cols, out)
    assert us > 0
    got = out.cpu().numpy()
    bad = np.argwhere((got != ref).any(axis=2))
    assert bad.size == 0, f"{len(bad)} queries differ, first {bad[:3]}: got {got[tuple(bad[0])]} ref {ref[tuple(bad[0])]}"


@pytest.mark.parametrize("mode,M,N,cols,rows", [(0, 50, 7, 1241, 376), (0, 5, 1, 1241, 376), (0, 40, 60, 60, 45), (0, 64, 200, 74, 376),
                                                 (1, 30, 9, 1241, 376), (0, 33, 0, 1241, 376), (1, 12, 0, 640, 480)])
def test_hamming_match_batched_sparse_and_narrow(hip_lib, mode, M, N, cols, rows):
    """edge shapes: almost empty hash grids (most cells empty, windows whose neighbours in bin order lie rows away), grids of
    1-3 cell columns (a window covers whole rows), a single train feature, none at all"""
    import torch
    rng = np.random.default_rng(100 + M + N + cols)
    B = 4
    td = rng.integers(0, 256, (B, max(N, 1), 32), dtype=np.uint8)[:, :N]
    qd = rng.integers(0, 256, (B, M, 32), dtype=np.uint8)
    txy = np.floor(rng.uniform(0, 1, (B, N, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    qxy = (rng.uniform(0, 1, (B, M, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    if N:
        # queries on top of / right beside train features, so that windows are not all empty
        k = min(M, N)
        qxy[:, :k] = txy[:, rng.integers(0, N, k)] + rng.uniform(-20, 20, (B, k, 2)).astype(np.float32)
        td[0] = td[0, 0]            # problem 0: all descriptors equal (ties -> lowest index)
    tf = np.zeros((B, N), np.uint8)
    if N > 3:
        tf[1, ::3] = 1
    ref = _hamming_ref_np(qd, qxy, td, txy, tf, 625.0, mode, rows) if N else np.tile(np.array([-1, 0x7FFFFFFF, -1, 0x7FFFFFFF], np.int32), (B, M, 1))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = torch.full((B, M, 4), 7, dtype=torch.int32, device="cuda")
    hip_lib.hamming_match_batched(t(qd), t(qxy), t(td.reshape(B, N, 32)), t(txy), t(tf), 625.0, mode, rows, cols, out)
    got = out.cpu().numpy()
    bad = np.argwhere((got != ref).any(axis=2))
    assert bad.size == 0, f"{len(bad)} queries differ, first {bad[:3]}: got {got[tuple(bad[0])]} ref {ref[tuple(bad[0])]}"


@pytest.mark.parametrize("M,N", [(200, 700), (1000, 1500)])
def test_hamming_row_mode_fractional_and_out_of_range_rows(hip_lib, M, N):
    """row mode walks row BINS; a train feature whose y is not an in-range integer row (fractional, above / below the image, NaN) must still be
    held to the reference's own comparison `y >= start_y && y <= end_y` (lvt_image_features_struct.cpp:133).  Problem 0: integer rows only (the
    walk without comparisons), 1: every kind mixed, 2: all fractional, 3: one single marked feature"""
    import torch
    rng = np.random.default_rng(5 + M)
    B, rows, cols = 4, 376, 1241
    td = rng.integers(0, 256, (B, N, 32), dtype=np.uint8)
    qd = rng.integers(0, 256, (B, M, 32), dtype=np.uint8)
    txy = np.floor(rng.uniform(0, 1, (B, N, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    qxy = (rng.uniform(0, 1, (B, M, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    txy[1, : N // 3, 1] += rng.uniform(0, 1, N // 3).astype(np.float32)            # fractional
    txy[1, N // 3: N // 3 + 40, 1] = rng.uniform(-9, 0, 40).astype(np.float32)     # above the image (bin 0)
    txy[1, N // 3 + 40: N // 3 + 80, 1] = rng.uniform(rows, rows + 9, 40).astype(np.float32)   # below it (last bin)
    txy[1, N // 3 + 80: N // 3 + 90, 1] = np.float32(np.nan)
    txy[1, N // 3 + 90: N // 3 + 100, 1] = np.float32(rows)                        # the row `end_y` may reach
    txy[2, :, 1] += rng.uniform(0.01, 0.99, N).astype(np.float32)
    txy[3, 17, 1] += np.float32(0.5)
    qxy[:, :30, 1] = rng.uniform(0, 4, (B, 30)).astype(np.float32)                 # queries at both image borders
    qxy[:, 30:60, 1] = rng.uniform(rows - 4, rows + 3, (B, 30)).astype(np.float32)
    tf = (rng.uniform(0, 1, (B, N)) < 0.1).astype(np.uint8)
    ref = _hamming_ref_np(qd, qxy, td, txy, tf, 0.0, 1, rows)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = torch.zeros((B, M, 4), dtype=torch.int32, device="cuda")
    hip_lib.hamming_match_batched(t(qd), t(qxy), t(td), t(txy), t(tf), 0.0, 1, rows, cols, out)
    got = out.cpu().numpy()
    bad = np.argwhere((got != ref).any(axis=2))
    assert bad.size == 0, f"{len(bad)} queries differ, first {bad[:3]}: got {got[tuple(bad[0])]} ref {ref[tuple(bad[0])]}"


def _pnp_against_oracle(hip_lib, oracle_lib, prm, q0, p0, X, uv, tag, noise_level=False, gross_outliers=False):
    """one stand-alone solve on both sides: the chi2 > 5.991 gate edge by edge (inlier count, levels), the number of solve calls, the pose, no
    borderline decision on either side, and the gates laid open.  `noise_level`: a solve the oracle itself ends in noise-level decisions
    (n = 1, 2) -- the calls and the counters are then nobody's to hold, the marks and the pose are.  `gross_outliers`: the input has edges whose
    e^2 reaches 1e6 .. 2e10 (points behind the camera, outliers of 1e5 px), where an absolute 1e-10 lies below one ulp of e^2 (2^-52 e^2 > 1e-10
    from e^2 = 4.5e5 on): their bound grows by 64 ulp of e^2 -- the camera-frame form and px / pz - u differ by about ten roundings of e^2 -- and
    stays 1e-10 in front of the gate.  Returns (q, p, inliers, calls) of the HIP path."""
    qo, po, marks, _ = oracle_lib.pnp(prm, q0, p0, X, uv)
    calls_o, border_o, margin_o = oracle_lib.pnp.last_solve_calls, oracle_lib.pnp.last_borderline, oracle_lib.pnp.last_min_margin
    err_o = oracle_lib.pnp.last_err.copy()
    qh, ph, inl, calls = hip_lib.pnp(prm, q0, p0, X, uv)
    assert inl == int(marks.sum()), (tag, inl, int(marks.sum()))          # the chi2 > 5.991 gate, edge by edge
    if not noise_level:
        assert calls == calls_o, (tag, calls, calls_o)
    assert np.allclose(ph, po, rtol=0, atol=1e-7) and np.allclose(qh, qo, rtol=0, atol=1e-9), (tag, ph, po, qh, qo)
    # the gates laid open: k_pnp's edge errors (refined reciprocals, camera-frame form, FMA sums) against the oracle's px / pz - u,
    # edge by edge -- the deviation must stay two orders of magnitude inside the margin within which a decision is re-evaluated
    _, _, inl2, _, err_h, level_h, border_h = hip_lib.pnp_detail(prm, q0, p0, X, uv)
    assert inl2 == inl and np.array_equal(level_h == 0, marks == 1), tag
    if not noise_level:
        e2h = (err_h ** 2).sum(axis=1); e2o = (err_o ** 2).sum(axis=1)
        seen = (level_h == 0) | (marks == 0)      # (an edge demoted by the FIRST gate keeps the error of pass 1 on both sides)
        bound = 1e-10 + (2.0 ** -46 * e2o if gross_outliers else 0.0)
        dev = (np.abs(e2h - e2o) / bound)[seen].max() if seen.any() else 0.0
        assert dev < 1.0, (tag, dev)
        assert border_h == border_o == 0, (tag, border_h, border_o, margin_o)
    return qh, ph, inl, calls


def test_pnp_standalone(hip_lib, oracle_lib):
    """k_pnp vs the oracle's g2o-LM restatement on synthetic 2D-3D sets incl. outliers (chi2 gate exercised)"""
    import lvt_amd
    rng = np.random.default_rng(3)
    prm = lvt_amd.kitti_params()
    for trial in range(4):
        n = [12, 200, 777, 1500][trial]
        X = np.column_stack([rng.uniform(-20, 20, n), rng.uniform(-5, 5, n), rng.uniform(6, 60, n)])
        ang = rng.normal(0, 0.01, 3)
        q_true = np.array([1.0, *(ang / 2)]); q_true /= np.linalg.norm(q_true)
        p_true = rng.normal(0, 0.3, 3)
        w, x, y, z = q_true
        Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                       [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                       [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        Xc = (X - p_true) @ Rm
        uv = np.column_stack([prm.fx * Xc[:, 0] / Xc[:, 2] + prm.cx, prm.fy * Xc[:, 1] / Xc[:, 2] + prm.cy])
        uv = np.rint(uv + rng.normal(0, 0.4, uv.shape)).astype(np.float32)
        uv[:: 9] += 25.0                                            # gross outliers
        q0 = np.array([1.0, 0, 0, 0]); p0 = np.zeros(3)
        qh, ph, inl, calls = _pnp_against_oracle(hip_lib, oracle_lib, prm, q0, p0, X, uv, trial)
        assert 0 < calls <= 10, (trial, calls)
        assert np.linalg.norm(ph - p_true) < 0.05


def _compare_trace_prefix(tro, trh, n, tag):
    """the two LM traces (rows: lambda, chi2 at the estimate, chi2 of the trial, rho) trial by trial, up to the first noise-level trial of either.
    A trial whose chi2 equals the estimate's to ~13 digits (LM has converged; g2o keeps iterating to its count of 5) is accepted or rejected on
    the LAST BITS of two sums over all edges: rho = (chi2 - chi2') / scale with |chi2 - chi2'| ~ 1e-14 chi2.  No two summation orders -- g2o's,
    the oracle's, k_pnp's tree -- agree on that sign; the estimates they lead to differ by ~1e-11 m.  Such a decision ends the trial-by-trial
    comparison; everything before it is held.  Returns (compared trials, worst |chi2 deviation| / bound)."""
    k = min(trace_noise(tro), trace_noise(trh), len(tro), len(trh))
    tro_k, trh_k = tro[:k], trh[:k]
    assert np.array_equal(np.isnan(trh_k), np.isnan(tro_k)) and np.array_equal(np.isfinite(tro_k), np.isfinite(trh_k)), tag
    fin = np.isfinite(tro_k) & np.isfinite(trh_k)
    assert np.allclose(trh_k[:, 0], tro_k[:, 0], rtol=1e-6, atol=0), (tag, trh_k[:, 0], tro_k[:, 0])
    # the two chi2 columns, the direct output of the sweep (log_ge1, rcp_nr) and of block_sum's tree.  The robust kernel d^2 log(1 + e^2 / d^2) has
    # slope <= 1, so an edge's term deviates by no more than its e^2 does (1e-10, test_pnp_standalone); the second term is the rounding of a sum of
    # up to 4 096 terms (4096 * 2^-53 = 4.5e-13)
    worst = 0.0
    for c in (1, 2):
        f = fin[:, c]
        bound = n * 1e-10 + 1e-12 * np.abs(tro_k[f, c])
        d = np.abs(trh_k[f, c] - tro_k[f, c])
        assert (d <= bound).all(), (tag, c, trh_k[f, c], tro_k[f, c], d / bound)
        if d.size:
            worst = max(worst, float((d / bound).max()))
    ok = fin[:, 3]
    # rho = (chi2 - chi2') / scale: compared relative to the chi2 values it is the difference of
    tol = 1e-9 * (np.abs(tro_k[ok, 1]) + np.abs(tro_k[ok, 2]) + 1.0) / np.maximum(np.abs(tro_k[ok, 1] - tro_k[ok, 2]), 1e-300) * np.abs(tro_k[ok, 3]) + 1e-9
    assert (np.abs(trh_k[ok, 3] - tro_k[ok, 3]) <= tol).all(), (tag, trh_k[ok, 3], tro_k[ok, 3])
    assert np.array_equal(trh_k[ok, 3] > 0, tro_k[ok, 3] > 0), tag
    return k, worst


def _pnp_hard_table(hip_lib, oracle_lib, table):
    """Trial by trial k_pnp must take the oracle's decisions -- same number of trials, the same ones rejected (rho <= 0: lambda *= ni, the estimate
    popped, the rejected trial's edge errors left in front of the 5.991 gate), Terminate at the same place, NaN steps (|delta| > 1 under
    sqrt(1 - |delta|^2)) rejected the same way -- with lambda, both chi2 and rho agreeing to rounding.  Returns the table's tally."""
    import lvt_amd
    prm = lvt_amd.kitti_params()
    t = dict(rej=0, term=0, nan=0, noise=0, full=0, full_rej=0, full_term=0, full_nan=0, chi2_ratio=0.0)
    for case in table:
        X, uv, q0, p0 = _pnp_hard_case(prm, *case)
        qo, po, marks, tro = oracle_lib.pnp(prm, q0, p0, X, uv)
        so = (oracle_lib.pnp.last_trials, oracle_lib.pnp.last_rejections, oracle_lib.pnp.last_terminates)
        calls_o = oracle_lib.pnp.last_solve_calls
        qh, ph, inl, calls, trh, sh = hip_lib.pnp_trace(prm, q0, p0, X, uv)
        k, ratio = _compare_trace_prefix(tro, trh, len(X), case)
        if k == len(tro) == len(trh):     # (no noise-level trial: the first case of PNP_HARD has one at its last trial)
            assert sh == so, (case, sh, so)
            assert calls == calls_o, (case, calls)
            t["full"] += 1
            t["full_rej"] += so[1]; t["full_term"] += so[2]; t["full_nan"] += int(np.isnan(tro).any())
        else:
            t["noise"] += 1
        assert inl == int(marks.sum()), (case, inl)
        assert np.allclose(ph, po, rtol=1e-7, atol=1e-7, equal_nan=True) and np.allclose(qh, qo, atol=1e-8, equal_nan=True), (case, ph, po)
        t["rej"] += so[1]; t["term"] += so[2]; t["nan"] += int(np.isnan(tro).any())
        t["chi2_ratio"] = max(t["chi2_ratio"], ratio)
        print(f"pnp hard case {case}: {k} of {len(tro)} trials compared, oracle (trials, rejections, terminates) {so}, chi2 deviation / bound {ratio:.2e}")
    return t


def test_pnp_rejected_trials_terminate_and_nan_steps(hip_lib, oracle_lib):
    """the hardest branch of g2o's Levenberg-Marquardt (lvt_pnp_solver.cpp:105-117): priors 1.5 - 10 m and 10 - 170 degrees off with
    30 - 50 % gross outliers (_pnp_hard_table)"""
    t = _pnp_hard_table(hip_lib, oracle_lib, PNP_HARD)
    # (the cases compared to their last trial must themselves cover the three branches)
    assert t["rej"] > 0 and t["term"] > 0 and t["nan"] > 0 and t["full"] >= 3 and t["full_rej"] > 0 and t["full_term"] + t["full_nan"] > 0, t


def test_pnp_hard_branches_above_the_staging_limit(hip_lib, oracle_lib):
    """the same branches at n = 1600, 2500, 4096: above PNP_STAGE_MAX pnp_solve leaves points, observations, levels and errors in global memory and
    the inactive lanes' sink behind the last edge's error.  Rejected trials there -- pop() leaves the rejected trial's errors in front of the
    5.991 gate -- NaN steps and Terminates, decision by decision."""
    assert all(c[1] > PNP_STAGE_MAX for c in PNP_HARD_UNSTAGED)
    t = _pnp_hard_table(hip_lib, oracle_lib, PNP_HARD_UNSTAGED)
    assert t["full"] >= 3 and t["rej"] > 0 and t["nan"] > 0 and t["term"] > 0, t


_EDGE_CASES = [(name, n) for name in PNP_INTRINSICS for n in PNP_EDGE_COUNTS]


@pytest.mark.parametrize("name,n", _EDGE_CASES, ids=[f"{name}-n{n}" for name, n in _EDGE_CASES])
def test_pnp_edge_counts(hip_lib, oracle_lib, name, n):
    """k_pnp at the edge counts where its structure changes -- below 8 edges (H of rank < 6 for n <= 2), a wavefront (pnp_sweep's early return,
    block_sum's inactive arm), PNP_THREADS, one sweep iteration, PNP_STAGE_MAX (LDS staging / global memory), NF_MAX -- under KITTI's, TUM's
    (fx != fy) and EuRoC's intrinsics; the oracle takes no borderline gate decision on any of them (test_case_tables.py)"""
    prm, X, uv, q0, p0 = pnp_edge_case(name, n)
    if n == 0:      # nothing to solve: the normalised prior comes back, no call, no inlier, no error from the entry point
        for q_in in (q0, np.array([-2.0, 0, 0, 0])):
            qh, ph, inl, calls = hip_lib.pnp(prm, q_in, p0, X, uv)
            assert (inl, calls) == (0, 0) and np.array_equal(qh, [1, 0, 0, 0]) and np.array_equal(ph, [0, 0, 0]), (qh, ph, inl, calls)
        qo, po, marks, tro = oracle_lib.pnp(prm, q0, p0, X, uv)
        assert oracle_lib.pnp.last_solve_calls == 0 and len(marks) == 0 and np.array_equal(qo, qh) and np.array_equal(po, ph)
        return
    noise_level = n <= 2
    _pnp_against_oracle(hip_lib, oracle_lib, prm, q0, p0, X, uv, (name, n), noise_level=noise_level)
    _, _, _, tro = oracle_lib.pnp(prm, q0, p0, X, uv)
    so = (oracle_lib.pnp.last_trials, oracle_lib.pnp.last_rejections, oracle_lib.pnp.last_terminates)
    _, _, _, _, trh, sh = hip_lib.pnp_trace(prm, q0, p0, X, uv)
    k, ratio = _compare_trace_prefix(tro, trh, n, (name, n))
    assert k >= min(3, len(tro)), (name, n, k, len(tro))      # (n = 1: the oracle's first noise-level trial is its fourth)
    if k == len(tro) == len(trh):
        assert sh == so, (name, n, sh, so)
    print(f"pnp {name} n={n}: {k} of {len(tro)} trials compared, chi2 deviation / bound {ratio:.2e}")


def test_pnp_normalises_its_prior_and_survives_points_behind_the_camera(hip_lib, oracle_lib):
    """SE3Quat's constructor normalises the prior and flips it to w >= 0: q, -q, 3 q and an unnormalised quaternion with w < 0 are one rotation and
    must give one solve, on inputs with 10 % of the points behind the camera (pcz < 0: g2o has no cheirality test) below and above the
    staging limit; and outliers graded 1 .. 1e5 px, log_ge1's argument range"""
    import lvt_amd
    prm = lvt_amd.kitti_params()
    for label, X, uv, priors, p0 in pnp_prior_cases(prm):
        got = [_pnp_against_oracle(hip_lib, oracle_lib, prm, q0, p0, X, uv, (label, j), gross_outliers=True) for j, q0 in enumerate(priors)]
        for j, (qh, ph, inl, calls) in enumerate(got[1:]):
            assert (inl, calls) == got[0][2:], (label, j + 1, inl, calls, got[0][2:])
            assert np.allclose(ph, got[0][1], rtol=0, atol=1e-7) and np.allclose(qh, got[0][0], rtol=0, atol=1e-9), (label, j + 1)
        if label.startswith("behind"):
            assert (X[:, 2] < 0).sum() >= len(X) // 20
        _, _, _, tro = oracle_lib.pnp(prm, priors[-1], p0, X, uv)
        _, _, _, _, trh, _ = hip_lib.pnp_trace(prm, priors[-1], p0, X, uv)
        k, ratio = _compare_trace_prefix(tro, trh, len(X), label)
        print(f"pnp {label}: {k} of {len(tro)} trials compared, chi2 deviation / bound {ratio:.2e}")


def test_pnp_edge_planted_on_the_chi2_threshold(hip_lib, oracle_lib):
    """an edge whose squared error sits ON the 5.991 gate: one 3-D point is moved (bisection on the ORACLE's decision) until the oracle's
    e^2 for that edge is within 1e-9 of the threshold, once just below and once just above.  k_pnp must notice the edge (borderline
    counter), re-evaluate it in the reference's operation order, and demote / keep exactly what the oracle does on either side."""
    import lvt_amd
    rng = np.random.default_rng(11)
    prm = lvt_amd.kitti_params()
    q0 = np.array([1.0, 0, 0, 0]); p0 = np.zeros(3)
    X, uv = _pnp_case(rng, prm, 400)
    d = np.array([0.0, 1.0, 0.0])                   # the edge's point moves along y: its v-error grows with it

    def oracle_e2(k, s):
        Xs = X.copy(); Xs[k] += s * d
        oracle_lib.pnp(prm, q0, p0, Xs, uv)
        return float((oracle_lib.pnp.last_err[k] ** 2).sum()), Xs

    def closest(k, s):          # how near any gate decision of the oracle came to the threshold with edge k's point moved by s
        oracle_e2(k, s)
        return oracle_lib.pnp.last_min_margin

    planted = None
    for k in (5, 6, 7, 8, 10, 11, 12):              # inlier edges (the gross outliers sit at 0, 9, 18, ...)
        lo, hi = 0.0, 2.0
        if not (oracle_e2(k, lo)[0] < 5.991 < oracle_e2(k, hi)[0]):
            continue
        for _ in range(200):                        # bisection on "edge k ends above the threshold": converges on the point where one of the
            mid = 0.5 * (lo + hi)                   # two gates sees its e^2 cross 5.991 (the first gate's flip makes the final error jump)
            if oracle_e2(k, mid)[0] > 5.991:
                hi = mid
            else:
                lo = mid
            if hi - lo < 1e-13:
                break
        if closest(k, lo) < 1e-9 and closest(k, hi) < 1e-9:
            planted = (k, lo, hi)
            break
    assert planted is not None, "no edge could be planted on the threshold"
    k, lo, hi = planted
    kept = []
    for s in (lo, hi):
        e2, Xs = oracle_e2(k, s)
        qo, po, marks, _ = oracle_lib.pnp(prm, q0, p0, Xs, uv)
        assert oracle_lib.pnp.last_borderline >= 1 and oracle_lib.pnp.last_min_margin < 1e-9
        qh, ph, inl, calls, err_h, level_h, border_h = hip_lib.pnp_detail(prm, q0, p0, Xs, uv)
        assert border_h >= 1, "k_pnp did not notice the edge on the threshold"
        assert np.array_equal(level_h == 0, marks == 1) and inl == int(marks.sum()), (s, e2, level_h[k], marks[k])
        assert calls == oracle_lib.pnp.last_solve_calls
        assert np.allclose(ph, po, rtol=0, atol=1e-7) and np.allclose(qh, qo, atol=1e-9)
        kept.append((int(marks[k]), e2))
    assert kept[0] != kept[1]       # the two sides really differ: the edge is kept on one side and demoted (or re-estimated) on the other


def test_rectify_matches_the_oracle(hip_lib):
    """k_rectify_map / k_rectify vs the oracle's restatement of cv::initUndistortRectifyMap + cv::remap with the EuRoC cam0 /
    cam1 calibration of the reference's example: maps bit-identical (same fp64 recurrence), rectified images identical"""
    from oracle import pyoracle as O
    from test_oracle_primitives import EUROC_L
    cams = [EUROC_L, dict(K=[457.587, 0.0, 379.999, 0.0, 456.134, 255.238, 0.0, 0.0, 1.0],
                          D=[-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0],
                          R=[0.9999633526194376, -0.003625811871560086, 0.007755443660172947, 0.003680398547259526, 0.9999684752771629,
                             -0.007035845251224894, -0.007729688520722713, 0.007064130529506649, 0.999945173484644],
                          P=EUROC_L["P"])]
    rng = np.random.default_rng(4)
    for c in cams:
        r = hip_lib.Rectifier(c["K"], c["D"], c["R"], c["P"], 752, 480)
        m1, m2 = r.maps()
        o1, o2 = O.init_undistort_rectify_map(c["K"], c["D"], c["R"], c["P"], 752, 480)
        assert np.array_equal(m1, o1) and np.array_equal(m2, o2)
        for kind in ("noise", "smooth"):
            img = rng.integers(0, 256, (480, 752), dtype=np.uint8)
            if kind == "smooth":
                yy, xx = np.mgrid[0:480, 0:752]
                img = ((np.sin(xx / 17.0) + np.cos(yy / 11.0)) * 60 + 128).astype(np.uint8)
            assert np.array_equal(r.rectify(img), O.remap_bilinear(img, o1, o2)), kind
        r.close()
