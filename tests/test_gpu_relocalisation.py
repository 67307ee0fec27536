"""-m gpu: the relocalisation stages through their entry points (k_reloc.hip) against tests/reloc_util.py, the numpy restatement of the definition in
include/lvt_amd_ext.h.  The matcher: indices and distances equal, query by query.  The solve: counts, best hypothesis, inlier list and the hypothesis
pose bit for bit; the refined pose within the bounds test_gpu_primitives.py holds lvt_amd_pnp to against pyoracle.pnp."""
import ctypes

import numpy as np
import pytest

import lvt_amd
import reloc_util as RU

pytestmark = pytest.mark.gpu

SENTINEL = -77


def _desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _match(hip_lib, q, t):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda() if len(a) else torch.zeros((0, 32), dtype=torch.uint8, device="cuda")
    out = torch.full((max(len(q), 1), 4), SENTINEL, dtype=torch.int32, device="cuda")
    us = hip_lib.reloc_match_device(dev(q), dev(t), out)
    assert us > 0 or len(q) == 0
    return out.cpu().numpy()[:len(q)]


def _hold_match(hip_lib, q, t, tag):
    ref = RU.global_match(q, t)
    got = _match(hip_lib, q, t)
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert bad.size == 0, f"{tag}: {bad.size} queries differ, first {bad[:3].tolist()}: got {got[bad[0]].tolist()} ref {ref[bad[0]].tolist()}"
    return ref


MATCH_SHAPES = [(n, 65) for n in (0, 1, 255, 256, 257)] + [(257, m) for m in (0, 1, 2, 31, 32, 33)] + [(4096, 32768)]


@pytest.mark.parametrize("N,M", MATCH_SHAPES, ids=[f"N{n}-M{m}" for n, m in MATCH_SHAPES])
def test_matcher_shapes(hip_lib, oracle_lib, N, M):
    """N either side of a workgroup's 256 queries and at capacity; M = 0, 1, 2, slice - 1, slice, slice + 1, 2 slice + 1 (the slice of a map this small is
    32 points) and at capacity (32 slices of 1024).  Random descriptors with duplicates inside the map."""
    assert hip_lib.reloc_slice_length(M) == (1024 if M == 32768 else 32)
    rng = np.random.default_rng(1000 * N + M)
    q, t = _desc(rng, N), _desc(rng, M)
    if M > 4:
        t[M - 1] = t[0]                          # a duplicate pair as far apart as the map allows
    ref = _hold_match(hip_lib, q, t, f"N={N} M={M}")
    for i in range(0, N, max(N // 5, 1)):        # ... and the restatement is the oracle's top two
        assert tuple(ref[i]) == oracle_lib.hamming_top2(q[i], t), i


def test_matcher_planted_at_the_ends_the_cuts_and_in_ties(hip_lib):
    """M = 2 slice + 9 = 73 at slice 32, and M = 3 * 1024 + 5 at slice 96: the best match planted at index 0, at M - 1 and either side of every cut; a
    duplicate of the best inside its slice and in another slice (the tie goes to the lowest index whichever slice reports first); distances 0 and 256;
    first and second best in different slices."""
    for M in (73, 3 * 1024 + 5):
        s = hip_lib.reloc_slice_length(M)
        cuts = list(range(s, M, s))
        spots = sorted({0, M - 1} | {c - 1 for c in cuts} | set(cuts))
        rng = np.random.default_rng(M)
        t = _desc(rng, M)
        q = _desc(rng, 3 * len(spots) + 2)
        for k, i in enumerate(spots):
            t[i] = _desc(rng, 1)[0]
            q[3 * k] = t[i]                                           # distance 0 at the spot, nothing else near
            q[3 * k + 1] = t[i]; q[3 * k + 1][0] ^= 1                 # distance 1 at the spot ...
        ref = _hold_match(hip_lib, q[:-2], t, f"M={M} single")
        for k, i in enumerate(spots):
            assert ref[3 * k, 0] == i and ref[3 * k, 1] == 0 and ref[3 * k + 1, 0] == i and ref[3 * k + 1, 1] == 1
        # duplicates: the spot's descriptor once more in the same slice and once in the last slice
        t2 = t.copy()
        lo, hi = cuts[0] - 1, cuts[0]                                 # last point of slice 0, first of slice 1
        t2[lo - 3] = t2[lo]                                           # same slice, lower index wins
        t2[M - 2] = t2[hi]                                            # another slice, lower index (hi) wins
        ka, kb = spots.index(lo), spots.index(hi)
        ref = _hold_match(hip_lib, q[:-2], t2, f"M={M} duplicates")
        assert ref[3 * ka].tolist() == [lo - 3, 0, lo, 0] and ref[3 * kb].tolist() == [hi, 0, M - 2, 0]       # first and second best in different slices
        # distance 256: a query that is the complement of EVERY map descriptor (the map is one descriptor M times)
        t3 = np.repeat(t[:1], M, axis=0)
        q3 = np.stack([~t[0], t[0]])
        ref = _hold_match(hip_lib, q3, t3, f"M={M} constant map")
        assert ref.tolist() == [[0, 256, 1, 256], [0, 0, 1, 0]]


# ---- the solve ------------------------------------------------------------------------------------------------------------------------------------
def _rot(rng, angle):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def problem(seed, n, n3=None, outliers=0.0, noise=0.3, prm=None):
    """n correspondences of a camera at a random pose two metres and 0.4 rad from the origin: world points, observations rounded to fp32 with `noise`
    px of error, camera-frame points with millimetres of error for the first n3; a share of gross outliers (observation and camera-frame point)"""
    prm = prm or lvt_amd.kitti_params()
    rng = np.random.default_rng(seed)
    R, t = _rot(rng, 0.4), rng.normal(0, 1.2, 3)
    pc = np.column_stack([rng.uniform(-12, 12, n), rng.uniform(-3, 3, n), rng.uniform(5, 40, n)])
    X = pc @ R.T + t
    uv = np.column_stack([prm.fx * pc[:, 0] / pc[:, 2] + prm.cx, prm.fy * pc[:, 1] / pc[:, 2] + prm.cy]) + rng.normal(0, noise, (n, 2))
    pcn = pc + rng.normal(0, 0.002, pc.shape) * (noise > 0)
    bad = rng.random(n) < outliers
    uv[bad] += rng.uniform(30, 200, (int(bad.sum()), 2))
    pcn[bad] += rng.normal(0, 3.0, (int(bad.sum()), 3))
    has = np.zeros(n, bool)
    has[:n if n3 is None else n3] = True
    return prm, X, uv.astype(np.float32), pcn, has, (R, t)


def _hold_solve(hip_lib, oracle_lib, prm, X, uv, pc, has, cfg=None, tag=""):
    cfg = cfg or {}
    ref = RU.solve(prm, X, uv, pc, has, cfg, pnp=oracle_lib.pnp)
    res, counts, inl, hR, ht = hip_lib.reloc_solve(prm, X, uv, pc, has, lvt_amd.RelocConfig(**cfg))
    print(tag, "status", res.status, ref["status"], "best", res.best_hypothesis, res.n_hyp_inliers, "refined", res.n_refined_inliers, ref["n_refined_inliers"],
          "count mismatches", int((counts != ref["counts"]).sum()))
    assert np.array_equal(counts, ref["counts"]), (tag, np.flatnonzero(counts != ref["counts"])[:5], counts[counts != ref["counts"]][:5], ref["counts"][counts != ref["counts"]][:5])
    assert (res.n_corr, res.n_with_point, res.best_hypothesis, res.n_hyp_inliers) == (ref["n_corr"], ref["n_with_point"], ref["best_hypothesis"], ref["n_hyp_inliers"]), tag
    assert res.status == ref["status"], (tag, res.status, ref["status"])
    if res.status in (0, 3):
        assert np.array_equal(inl, ref["inliers"]), tag
        assert np.array_equal(hR, ref["hyp_R"]) and np.array_equal(ht, ref["hyp_t"]), (tag, hR - ref["hyp_R"], ht - ref["hyp_t"])     # bit for bit
        assert res.n_refined_inliers == ref["n_refined_inliers"], tag
        assert np.allclose(res.p, ref["p"], rtol=0, atol=1e-7) and np.allclose(res.q, ref["q"], rtol=0, atol=1e-9), (tag, res.p, ref["p"], res.q, ref["q"])
        w, x, y, z = res.q
        assert np.allclose(res.R, [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], atol=1e-14) and np.array_equal(res.t, res.p)
    else:
        assert not res.q.any() and not res.p.any() and not res.R.any() and not res.t.any() and res.n_refined_inliers == 0
    return res, ref


@pytest.mark.parametrize("n", [0, 2, 3, 64, 65, 4096])
def test_solve_sizes(hip_lib, oracle_lib, n):
    """n either side of a wavefront's 64 lanes, at capacity (more edges than the solver stages in LDS), and too few for a hypothesis.  40 in 100
    correspondences are gross outliers."""
    prm, X, uv, pc, has, (R, t) = problem(n, n, outliers=0.4)
    res, ref = _hold_solve(hip_lib, oracle_lib, prm, X, uv, pc, has, {"min_inliers": 3 if n < 64 else 30}, f"n={n}")
    assert res.status == (1 if n < 3 else 0 if n >= 64 else res.status)
    if n >= 64:
        assert np.linalg.norm(res.p - t) < 0.05 and 0.45 * n < res.n_refined_inliers < 0.75 * n


@pytest.mark.parametrize("n3", [0, 2, 3])
def test_solve_few_camera_points(hip_lib, oracle_lib, n3):
    """n3 = 3: two of three draws coincide in most hypotheses (they score 0); the others are all one triad"""
    prm, X, uv, pc, has, _ = problem(40 + n3, 64, n3=n3, noise=0.1)
    res, ref = _hold_solve(hip_lib, oracle_lib, prm, X, uv, pc, has, None, f"n3={n3}")
    assert res.status == (1 if n3 < 3 else 0)
    if n3 == 3:
        assert (ref["counts"] == 0).sum() > 128 and (ref["counts"] > 0).sum() > 16


@pytest.mark.parametrize("n_hyp", [1, 4, 5, 1024])
def test_solve_hypothesis_counts(hip_lib, oracle_lib, n_hyp):
    """a workgroup scores four hypotheses: one, a full workgroup, one more, the limit"""
    prm, X, uv, pc, has, _ = problem(7, 200, outliers=0.2)
    _hold_solve(hip_lib, oracle_lib, prm, X, uv, pc, has, {"n_hypotheses": n_hyp, "seed": 2 ** 64 - 3}, f"n_hyp={n_hyp}")


def test_solve_degenerate_and_poisoned_inputs(hip_lib, oracle_lib):
    prm, X, uv, pc, has, _ = problem(21, 96, noise=0.2)
    # all points on one line, in both sets: every triad is degenerate, nothing scores
    line = np.linspace(1, 9, 96)[:, None] * np.array([[0.1, 0.2, 1.0]])
    res, ref = _hold_solve(hip_lib, oracle_lib, prm, line + [1.0, 2, 3], uv, line, has, None, "collinear")
    assert res.status == 2 and res.n_hyp_inliers == 0 and res.best_hypothesis == 0
    # points behind the camera whose observations fit: pcz <= 0 is never an inlier
    Xb, pcb = X.copy(), pc.copy()
    Rm, t = problem(21, 96, noise=0.2)[5]
    pcb[60:, 2] *= -1; pcb[60:, :2] *= -1                     # (x, y, z) -> -(x, y, z): the same pixel, behind the camera
    Xb[60:] = pcb[60:] @ Rm.T + t
    hb = has.copy(); hb[60:] = False
    res, ref = _hold_solve(hip_lib, oracle_lib, prm, Xb, uv, pcb, hb, None, "behind")
    assert res.status == 0 and res.n_hyp_inliers <= 60
    # a NaN camera-frame point and a NaN world point: hypotheses drawn from them have no inlier, the poisoned correspondences are nobody's inlier
    Xn, pcn = X.copy(), pc.copy()
    pcn[5, 1] = np.nan; Xn[9, 2] = np.nan; pcn[11] = np.inf
    res, ref = _hold_solve(hip_lib, oracle_lib, prm, Xn, uv, pcn, has, None, "nan")
    assert res.status == 0 and 9 not in ref["inliers"] and (ref["counts"] == 0).any()


def test_solve_ties_go_to_the_lowest_hypothesis(hip_lib, oracle_lib):
    prm, X, uv, pc, has, _ = problem(3, 64, noise=0.0)      # exact points: many hypotheses hold every correspondence (the observations' fp32 rounding aside)
    res, ref = _hold_solve(hip_lib, oracle_lib, prm, X, uv, pc, has, {"gate_px2": 1.0}, "ties")
    top = np.flatnonzero(ref["counts"] == ref["counts"].max())
    assert len(top) >= 2 and res.best_hypothesis == top[0]


def test_solve_gate_boundary(hip_lib, oracle_lib):
    """edges planted either side of gate_px2 under the one hypothesis of the call: they have no camera-frame point, so they do not change it"""
    gate = 9.0
    cfg = {"gate_px2": gate, "n_hypotheses": 1, "seed": 4}
    prm, X, uv, pc, has, _ = problem(5, 80, noise=0.05)
    first = RU.solve(prm, X, uv, pc, has, cfg)
    assert first["n_hyp_inliers"] >= 60
    R, t = first["hyp_R"], first["hyp_t"]
    k = 16
    Xp = X[:k] + 0.5
    pcp = (Xp - t) @ R
    base = np.column_stack([prm.fx * pcp[:, 0] / pcp[:, 2] + prm.cx, prm.fy * pcp[:, 1] / pcp[:, 2] + prm.cy])
    off = 3.0 * (1 + 1e-3 * np.where(np.arange(k) % 2, 1.0, -1.0))      # |e| = 3 (1 -+ 1e-3) px: e.e = 9 (1 -+ 2e-3), fp32 rounding of u is 3e-5 px
    uvp = base + np.column_stack([off, np.zeros(k)])
    X2, uv2 = np.vstack([X, Xp]), np.vstack([uv, uvp.astype(np.float32)])
    pc2, has2 = np.vstack([pc, np.zeros((k, 3))]), np.concatenate([has, np.zeros(k, bool)])
    res, ref = _hold_solve(hip_lib, oracle_lib, prm, X2, uv2, pc2, has2, cfg, "gate")
    assert np.array_equal(ref["hyp_R"], first["hyp_R"]) and np.array_equal(ref["hyp_t"], first["hyp_t"])
    planted = np.isin(np.arange(80, 80 + k), ref["inliers"])
    assert planted.tolist() == [i % 2 == 0 for i in range(k)]


# ---- sequences: eight frames, a blackout, a later frame, the call ------------------------------------------------------------------------------------------
def _feed(sys_, world, sensor, i, u16=False):
    if sensor == 2:
        g, d = world.render_rgbd(i)
        if u16:
            return sys_.track(g, np.rint(d * 5000.0).astype(np.uint16), depth_scale=1.0 / 5000.0)
        return sys_.track(g, d)
    return sys_.track(*world.render_stereo(i))


def _lost_handle(hip_lib, kind, variant):
    """a handle that tracked frames 0 .. 7, went LOST on a flat frame and was then handed frame 8 + gap (it stays LOST and returns the last pose)"""
    from parity_util import make_case
    from test_reloc import SCENARIOS
    world, prm, sensor = make_case(kind, SCENARIOS[kind][0], 0.5)
    sys_ = hip_lib.LvtSystem.create(prm, sensor)
    if variant == "equalised":
        assert sys_.set_equalisation(hip_lib.Equalisation()) == 0
    u16 = variant == "depth16"
    flat = np.full((world.H, world.W), 110, np.uint8)
    f = 8 + SCENARIOS[kind][1]
    if variant == "in_flight":                       # the last three frames -- 7, the blackout, f -- are in flight together and drained before the call
        for i in range(7):
            _feed(sys_, world, sensor, i)
        last = world.render_stereo(7)
        held = [last, (flat, flat), world.render_stereo(f)]
        for a, b in held:
            assert sys_.track_async(a, b) == 0
        for _ in held:
            sys_.wait()
    else:
        for i in range(8):
            _feed(sys_, world, sensor, i, u16)
            assert sys_.get_state() == 2
        if sensor == 2:
            sys_.track(flat, np.zeros((world.H, world.W), np.uint16), depth_scale=1.0 / 5000.0) if u16 else sys_.track(flat, np.zeros((world.H, world.W), np.float32))
        else:
            sys_.track(flat, flat)
        assert sys_.get_state() == 3
        _feed(sys_, world, sensor, f, u16)
    assert sys_.get_state() == 3 and sys_.last_error() == ""
    return sys_, world, prm, sensor, f


def _restated(sys_, oracle_lib, world, prm, sensor, f, cfg, variant):
    """the restatement fed the map read back from the handle and the features of the frame it was handed last.  A LOST frame's features are nobody's to
    read back (lvt_amd_get_features reports none for it, as the oracle does), so they are the oracle's of the same images -- the features every parity test
    holds the feature stage to, bit for bit; of an equalising handle: of the equalised planes read back from it."""
    xyz, _, _, desc = sys_.map()
    assert len(sys_.features(0)[0]) == 0
    if sensor == 2:
        g, d = world.render_rgbd(f)
        if variant == "depth16":
            d = (np.rint(d * 5000.0).astype(np.uint16).astype(np.float32) * np.float32(1.0 / 5000.0)).astype(np.float32)
        xy, _, de, _ = oracle_lib.compute_features(g, prm)
        dep = d[xy[:, 1].astype(int), xy[:, 0].astype(int)].astype(np.float32)      # (no distortion in this world: the stored coordinates are the raw ones)
        keep = (dep >= np.float32(prm.near_plane_distance)) & (dep <= np.float32(prm.far_plane_distance))
        return RU.relocalise(prm, sensor, xyz, desc, xy[keep], de[keep], depth=dep[keep], cfg=cfg, pnp=oracle_lib.pnp)
    L, R = world.render_stereo(f)
    if variant == "equalised":
        L, R = (np.ascontiguousarray(sys_.plane(e, 5)[:world.H, :world.W]) for e in (0, 1))
    xy, _, de, _ = oracle_lib.compute_features(L, prm)
    xyr, _, der, _ = oracle_lib.compute_features(R, prm)
    return RU.relocalise(prm, sensor, xyz, desc, xy, de, right=(xyr, der), cfg=cfg, pnp=oracle_lib.pnp)


INT_FIELDS = ("status", "n_features", "n_map", "n_matched", "n_corr", "n_with_point", "best_hypothesis", "n_hyp_inliers", "n_refined_inliers")
SEQUENCE_CASES = [("kitti", "sync"), ("euroc", "sync"), ("tum", "sync"), ("tum", "depth16"), ("kitti", "in_flight"), ("kitti", "equalised")]


@pytest.mark.parametrize("kind,variant", SEQUENCE_CASES, ids=[f"{k}-{v}" for k, v in SEQUENCE_CASES])
def test_sequence_relocalises_like_the_restatement(hip_lib, oracle_lib, kind, variant):
    """every integer field of the result equal to the restatement's; the pose within lvt_amd_pnp's bounds against pyoracle.pnp; a dry run changes not one
    byte of the state; the committed state answers at once; the next frame tracks on in the old map's coordinates"""
    sys_, world, prm, sensor, f = _lost_handle(hip_lib, kind, variant)
    from test_reloc import SCENARIOS
    u16 = variant == "depth16"
    mi = SCENARIOS[kind][2]
    ref = _restated(sys_, oracle_lib, world, prm, sensor, f, {"min_inliers": mi}, variant)
    before = sys_.snapshot().to_bytes()
    frame_no = sys_.counts()["frame"]
    m_before = sys_.matches()
    dry = sys_.relocalise(dry_run=1, min_inliers=mi)
    print(kind, variant, {k: getattr(dry, k) for k in INT_FIELDS}, "ref", {k: ref[k] for k in INT_FIELDS})
    assert {k: getattr(dry, k) for k in INT_FIELDS} == {k: ref[k] for k in INT_FIELDS}
    assert dry.status == 0 and dry.n_features > 0
    assert np.allclose(dry.p, ref["p"], rtol=0, atol=1e-7) and np.allclose(dry.q, ref["q"], rtol=0, atol=1e-9), (dry.p, ref["p"], dry.q, ref["q"])
    assert sys_.get_state() == 3 and sys_.snapshot().to_bytes() == before                      # a dry run: not one byte
    res = sys_.relocalise(min_inliers=mi)
    assert bytes(memoryview(res)) == bytes(memoryview(dry))                                    # the same call, the same record
    q, p = sys_.pose()
    assert sys_.get_state() == 2 and np.array_equal(q, res.q) and np.array_equal(p, res.p)
    c = sys_.counts()
    assert c["frame"] == frame_no and c["map_size"] == ref["n_map"]
    assert all(np.array_equal(a, b) for a, b in zip(sys_.matches(), m_before))                 # the last frame's matches still answer
    assert np.linalg.norm(res.p - world.pose(f)[1]) < 0.1
    info = sys_.snapshot().info
    assert info["state"] == 2 and info["map_n"] == ref["n_map"]
    # the next frames track on from the committed pose, in the old map's coordinates
    for i in (f + 1, f + 2):
        R, t = _feed(sys_, world, sensor, i, u16)
        assert sys_.get_state() == 2 and sys_.last_error() == "", sys_.last_error()
        assert np.linalg.norm(t - world.pose(i)[1]) < 0.1, (i, t, world.pose(i)[1])
    assert sys_.counts()["frame"] == frame_no + 2
    sys_.close()


def test_relocalise_refusals_in_order(hip_lib):
    from parity_util import make_case
    world, prm, sensor = make_case("kitti", 0, 0.5)
    sys_ = hip_lib.LvtSystem.create(prm, sensor)
    L = hip_lib.load_library()
    res = lvt_amd.RelocResult()
    assert L.lvt_amd_relocalise(None, None, ctypes.byref(res)) == -1                           # a bad handle
    for call, words in ((lambda: L.lvt_amd_batch_relocalise(sys_._h, 0, None, ctypes.byref(res)), "not a batch"),
                        (lambda: L.lvt_amd_relocalise(sys_._h, ctypes.byref(lvt_amd.RelocConfig(n_hypotheses=0)), ctypes.byref(res)), "n_hypotheses"),
                        (lambda: L.lvt_amd_relocalise(sys_._h, None, ctypes.byref(res)), "has not seen a frame")):
        assert call() == -1
        assert words in sys_.last_error() and sys_.last_error().endswith("(nothing was changed)"), sys_.last_error()
    sys_.track(np.full((world.H, world.W), 110, np.uint8), np.full((world.H, world.W), 110, np.uint8))        # a frame, but nothing to map
    with pytest.raises(ValueError, match="min_inliers.*nothing was changed"):                 # a bad field comes before the empty map
        sys_.relocalise(min_inliers=2)
    with pytest.raises(ValueError, match="an empty map.*nothing was changed"):
        sys_.relocalise()
    sys_.close()
    sys_ = hip_lib.LvtSystem.create(prm, sensor)
    for i in range(2):
        sys_.track(*world.render_stereo(i))
    assert sys_.track_async(*world.render_stereo(2)) == 0
    with pytest.raises(ValueError, match="frames in flight.*nothing was changed"):
        sys_.relocalise()
    sys_.wait()
    sys_.close()
    batch = hip_lib.LvtBatch(prm, 2)
    with pytest.raises(ValueError, match="a batch handle.*nothing was changed"):
        lvt_amd._relocalise(batch._h, None, None, {})
    with pytest.raises(ValueError, match="no sequence 2.*nothing was changed"):
        batch.relocalise(2)
    with pytest.raises(ValueError, match="has not seen a frame"):
        batch.relocalise(1)
    batch.close()


def test_tracking_handle_against_its_own_features(hip_lib, oracle_lib):
    """any state is accepted: on a TRACKING handle the last frame's features CAN be read back, so here the restatement is fed nothing but what the handle
    itself returns -- map, left and right features -- and every integer field and the pose are held to it; the handle finds the pose it has"""
    from parity_util import make_case
    world, prm, sensor = make_case("kitti", 0, 0.5)
    sys_ = hip_lib.LvtSystem.create(prm, sensor)
    for i in range(5):
        sys_.track(*world.render_stereo(i))
    assert sys_.get_state() == 2
    xyz, _, _, desc = sys_.map()
    (xy, _, de), (xyr, _, der) = sys_.features(0), sys_.features(1)
    assert len(xy) > 100 and len(xyr) > 100
    ref = RU.relocalise(prm, sensor, xyz, desc, xy, de, right=(xyr, der), pnp=oracle_lib.pnp)
    q0, p0 = sys_.pose()
    res = sys_.relocalise(dry_run=1)
    assert {k: getattr(res, k) for k in INT_FIELDS} == {k: ref[k] for k in INT_FIELDS} and res.status == 0
    assert np.allclose(res.p, ref["p"], rtol=0, atol=1e-7) and np.allclose(res.q, ref["q"], rtol=0, atol=1e-9)
    tg = world.pose(4)[1]
    print("tracking handle: tracked pose off the ground truth by", np.linalg.norm(p0 - tg), "relocalised by", np.linalg.norm(res.p - tg), "inliers", res.n_refined_inliers)
    assert np.linalg.norm(res.p - tg) < 0.1 and sys_.get_state() == 2          # (the bound of every half-size world here)
    sys_.close()


def test_batch_relocalises_one_sequence_and_leaves_its_neighbours(hip_lib, oracle_lib):
    """a mixed batch of three stereo sequences (kitti seed 0, euroc seed 0, kitti seed 3) in lock-step: all go LOST on a flat frame, then each is handed
    its own later frame.  lvt_amd_batch_relocalise on sequence 1 and then on sequence 0: the result equals the restatement fed THAT sequence's map and
    frame (the per-sequence buffers, record and map copy are the right ones), the neighbours' snapshot bytes do not change, and only that sequence
    answers TRACKING; sequence 2 is never relocalised and stays LOST."""
    import torch
    from parity_util import make_case
    from test_reloc import SCENARIOS
    cases = [("kitti", 0, 8 + SCENARIOS["kitti"][1], 30), ("euroc", 0, 8 + SCENARIOS["euroc"][1], 10), ("kitti", 3, 8 + 40, 30)]
    worlds = [make_case(k, s, 0.5) for k, s, _, _ in cases]
    batch = hip_lib.LvtBatch.create_mixed([w[1] for w in worlds], 1)
    keep = []

    def step(frames):
        L, R, rows, cols, pitch = [], [], [], [], []
        for (world, prm, _), (l, r) in zip(worlds, frames):
            p = (world.W + 15) // 16 * 16
            dl, dr = (torch.zeros((world.H, p), dtype=torch.uint8, device="cuda") for _ in range(2))
            dl[:, :world.W] = torch.from_numpy(np.ascontiguousarray(l)).cuda(); dr[:, :world.W] = torch.from_numpy(np.ascontiguousarray(r)).cuda()
            keep.append((dl, dr))
            L.append(dl.data_ptr()); R.append(dr.data_ptr()); rows.append(world.H); cols.append(world.W); pitch.append(p)
        torch.cuda.synchronize()
        assert batch.track_device_async_mixed(L, R, rows, cols, pitch) == 0, batch.last_error()
        return batch.wait()
    for i in range(8):
        _, _, st = step([w[0].render_stereo(i) for w in worlds])
        assert list(st) == [2, 2, 2]
    flats = [(np.full((w[0].H, w[0].W), 110, np.uint8),) * 2 for w in worlds]
    step(flats)
    _, _, st = step([w[0].render_stereo(c[2]) for w, c in zip(worlds, cases)])
    assert list(st) == [3, 3, 3]
    for seq in (1, 0):
        (world, prm, sensor), (_, _, f, mi) = worlds[seq], cases[seq]
        others = [s for s in range(3) if s != seq]
        before = {s: batch.snapshot(s).to_bytes() for s in range(3)}
        snap = batch.snapshot(seq)
        solo = hip_lib.LvtSystem.create(prm, sensor)               # the sequence's map, read through a solo handle the snapshot is applied to
        assert solo.restore(snap) == 0
        xyz, _, _, desc = solo.map()
        solo.close()
        L, R = world.render_stereo(f)
        xy, _, de, _ = oracle_lib.compute_features(L, prm)
        xyr, _, der, _ = oracle_lib.compute_features(R, prm)
        ref = RU.relocalise(prm, sensor, xyz, desc, xy, de, right=(xyr, der), cfg={"min_inliers": mi}, pnp=oracle_lib.pnp)
        dry = batch.relocalise(seq, dry_run=1, min_inliers=mi)
        assert {k: getattr(dry, k) for k in INT_FIELDS} == {k: ref[k] for k in INT_FIELDS} and dry.status == 0, (seq, {k: getattr(dry, k) for k in INT_FIELDS}, {k: ref[k] for k in INT_FIELDS})
        assert {s: batch.snapshot(s).to_bytes() for s in range(3)} == before                        # a dry run: not one byte, of anyone
        res = batch.relocalise(seq, min_inliers=mi)
        assert res.status == 0 and np.allclose(res.p, ref["p"], rtol=0, atol=1e-7) and np.allclose(res.q, ref["q"], rtol=0, atol=1e-9)
        assert np.linalg.norm(res.p - world.pose(f)[1]) < 0.1
        after = {s: batch.snapshot(s) for s in range(3)}
        assert all(after[s].to_bytes() == before[s] for s in others), seq                           # the neighbours: untouched
        assert after[seq].info["state"] == 2 and after[seq].to_bytes() != before[seq]
    states = [batch.snapshot(s).info["state"] for s in range(3)]
    assert states == [2, 2, 3]
    # the next lock-step frame: the two relocalised sequences track on in their old maps' coordinates, the third stays LOST
    _, t, st = step([w[0].render_stereo(c[2] + 1) for w, c in zip(worlds, cases)])
    assert list(st) == [2, 2, 3], batch.last_error()
    t = np.asarray(t).reshape(3, 3)
    for s in (0, 1):
        assert np.linalg.norm(t[s] - worlds[s][0].pose(cases[s][2] + 1)[1]) < 0.1, (s, t[s])
    batch.close()
