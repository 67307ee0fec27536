"""CPU tier: the relocalisation search as tests/reloc_util.py restates it (include/lvt_amd_ext.h, RELOCALISATION) -- its stages against the oracle's
primitives and against answers worked out by hand, and the whole search on the synthetic worlds after a blackout."""
import ctypes
import os

import numpy as np
import pytest

import lvt_amd
import reloc_util as RU
from parity_util import make_case


def _desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


# ---- stage 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_global_match_is_hamming_top2_query_by_query(oracle_lib):
    rng = np.random.default_rng(11)
    for n_q, n_t in ((7, 0), (5, 1), (9, 2), (40, 300)):
        q, t = _desc(rng, n_q), _desc(rng, n_t)
        if n_t >= 300:
            t[17] = t[203] = q[3]                  # distance 0 twice: the lowest index first, its duplicate second
            t[250] = t[9]
            q[5] = ~t[9]                           # distance 256 to both copies of one descriptor
        rec = RU.global_match(q, t)
        for i in range(n_q):
            assert tuple(rec[i]) == oracle_lib.hamming_top2(q[i], t), (n_q, n_t, i)
    assert tuple(RU.global_match(_desc(rng, 1), _desc(rng, 0))[0]) == (-1, 0x7FFFFFFF, -1, 0x7FFFFFFF)


# ---- hand-checked answers -----------------------------------------------------------------------------------------------------------------------
def test_accept_rule_by_hand():
    assert RU.accept_match(2, 39, 50, 0.8, 30.0)             # 0.78 < 0.8
    assert not RU.accept_match(2, 40, 50, 0.8, 30.0)         # 0.8 < 0.8 fails: (float)40 / (float)50 rounds to the fp32 0.8 the threshold is
    assert not RU.accept_match(2, 0, 0, 0.8, 30.0)           # 0 / 0 is NaN
    assert RU.accept_match(2, 0, 1, 0.8, 30.0)
    assert RU.accept_match(1, 30, 0, 0.8, 30.0) and not RU.accept_match(1, 31, 0, 0.8, 30.0)   # one map point: d1 <= desc_th
    assert not RU.accept_match(0, 0, 0, 0.8, 30.0)


def test_mutual_filter_by_hand():
    # features 0, 2 and 3 claim map point 5; 2 and 3 at the same distance: the lower feature index keeps it.  Feature 1 fails the ratio.
    rec = np.array([[5, 30, 1, 100], [7, 90, 2, 100], [5, 20, 1, 100], [5, 20, 3, 100], [4, 10, 0, 100]], np.int32)
    feat, mp, n_matched = RU.correspondences(rec, 10, 0.8, 30.0)
    assert n_matched == 4 and feat.tolist() == [2, 4] and mp.tolist() == [5, 4]


def test_sampler_by_hand():
    def by_hand(seed, h, j, n3):
        x = (seed + (3 * h + j + 1) * 0x9E3779B97F4A7C15) % 2 ** 64
        x ^= x >> 30
        x = x * 0xBF58476D1CE4E5B9 % 2 ** 64
        x ^= x >> 27
        x = x * 0x94D049BB133111EB % 2 ** 64
        x ^= x >> 31
        return x % n3
    # seed 0, h 0, j 0 is the first output of splitmix64(0), a published value
    assert RU.sample(0, 0, 0, 2 ** 64) == 0xE220A8397B1DCDAF
    for seed, h, j, n3 in ((0, 0, 0, 3), (0, 0, 1, 3), (1, 255, 2, 4096), (2 ** 64 - 1, 1023, 2, 413), (12345678901234567890, 7, 1, 1)):
        assert RU.sample(seed, h, j, n3) == by_hand(seed, h, j, n3)


def test_triad_recovers_a_known_rigid_motion():
    # camera points on the axes; the world is the camera turned 90 degrees about z and moved by (1, 2, 3): R = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    a = np.array([[0.0, 0, 0], [2.0, 0, 0], [0.0, 3, 0], [1.0, 1, 5]])
    R_true = np.array([[0.0, -1, 0], [1.0, 0, 0], [0.0, 0, 1]]); t_true = np.array([1.0, 2, 3])
    b = np.array([R_true @ p + t_true for p in a])
    e1, e2, e3 = RU.triad(*a[:3])
    assert (e1, e2, e3) == ([1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0])
    for seed in range(40):                          # whichever three distinct samples a seed draws, exact inputs give the exact motion
        hyp = RU.hypothesis(seed, 0, np.arange(4), a, b)
        if hyp is not None:
            assert np.allclose(hyp[0], R_true, atol=1e-15) and np.allclose(hyp[1], t_true, atol=1e-14)
    assert sum(RU.hypothesis(s, 0, np.arange(4), a, b) is not None for s in range(40)) > 5


def test_every_degenerate_hypothesis_scores_zero():
    good = np.array([[0.0, 0, 1], [1.0, 0, 1], [0.0, 1, 1]])
    assert RU.triad(*good) is not None
    assert RU.triad(good[0], good[0] + [1e-6, 0, 0], good[2]) is None          # |p1 - p0|^2 = 1e-12: <= is degenerate
    assert RU.triad(good[0], good[0] + [1.1e-6, 0, 0], good[2]) is not None
    assert RU.triad(good[0], good[1], good[0] + [5.0, 0, 0]) is None           # collinear: e1 x (p2 - p0) = 0
    assert RU.triad(good[0], good[1], good[0] + [5.0, 1e-6, 0]) is None        # |e1 x (p2 - p0)|^2 = 1e-12
    # coincident samples: with n3 = 1 every hypothesis draws one correspondence three times
    assert RU.hypothesis(0, 0, np.arange(1), good, good) is None
    # a degenerate triad in EITHER set
    flat = good.copy(); flat[2] = [2.0, 0, 1]
    some = [h for h in range(64) if len({RU.sample(0, h, j, 3) for j in range(3)}) == 3]
    assert some and all(RU.hypothesis(0, h, np.arange(3), good, good) is not None for h in some)
    assert all(RU.hypothesis(0, h, np.arange(3), flat, good) is None and RU.hypothesis(0, h, np.arange(3), good, flat) is None for h in some)
    prm = lvt_amd.kitti_params()
    counts, _ = RU.score_all(0, 64, np.arange(3), flat, good, np.zeros((3, 2), np.float32), prm, 16.0)
    assert not counts.any()


def test_quaternion_of_a_rotation_matrix_by_hand():
    assert np.array_equal(RU.mat3_to_quat(np.eye(3)), [1.0, 0, 0, 0])
    assert np.allclose(RU.mat3_to_quat([[0.0, -1, 0], [1.0, 0, 0], [0.0, 0, 1]]), [np.sqrt(0.5), 0, 0, np.sqrt(0.5)], atol=1e-16)
    assert np.array_equal(RU.mat3_to_quat(np.diag([1.0, -1, -1])), [0.0, 1, 0, 0])       # trace -1: the branch on the largest diagonal element
    assert np.array_equal(RU.mat3_to_quat(np.diag([-1.0, -1, 1])), [0.0, 0, 0, 1])


# ---- the scenario: eight frames, a blackout, a later frame of the same scene -------------------------------------------------------------------------
# kind -> (seed of the half-size world, gap, min_inliers): the frame relocalised on is 8 + gap.  Chosen with the restatement itself, so that BOTH hold:
#  - it returns status 0 with at least 2 max(min_inliers, min_num_matches_for_tracking) refined inliers (kitti 155 of 60; euroc 47 of 20; tum 22 of 20);
#  - `far`, the share of map points whose projection under the last tracked pose lies more than twice tracking_radius from their projection under the true
#    pose, exceeds one half (kitti 0.92, euroc 0.56, tum 0.55): the frame path's search (one radius, two on its second pass) cannot reach those.
# The half-size euroc and tum worlds sway within a few decimetres and keep few features (maps of 108 and 1980 points, 120 and 290 features a frame): where most
# of the map has left the frame path's reach, 64 and 22 correspondences are left, so those two run with min_inliers = 10 (the field's range is >= 3; the
# success count is then max(10, 10) = 10 and the condition 20).  With the default 30 no seed 0 .. 6 and gap up to 260 meets both conditions.
SCENARIOS = {"kitti": (0, 48, 30), "euroc": (0, 164, 10), "tum": (1, 169, 10)}


def blackout_case(oracle_lib, kind):
    """(world, prm, sensor, oracle in state LOST, frame index to relocalise on)"""
    world, prm, sensor = make_case(kind, SCENARIOS[kind][0], 0.5)
    orc = oracle_lib.Oracle(prm, sensor)
    flat = np.full((world.H, world.W), 110, np.uint8)
    for i in range(8):
        orc.track_rgbd(*world.render_rgbd(i)) if sensor == 2 else orc.track(*world.render_stereo(i))
        assert orc.status == 2
    orc.track_rgbd(flat, np.zeros((world.H, world.W), np.float32)) if sensor == 2 else orc.track(flat, flat)
    assert orc.status == 3
    return world, prm, sensor, orc, 8 + SCENARIOS[kind][1]


def frame_features(oracle_lib, world, prm, sensor, f):
    """the features of frame f as the tracker's feature stage keeps them: (xy, desc, right or None, depth or None)"""
    if sensor == 2:
        g, d = world.render_rgbd(f)
        xy, _, de, _ = oracle_lib.compute_features(g, prm)
        dep = d[xy[:, 1].astype(int), xy[:, 0].astype(int)].astype(np.float32)
        keep = (dep >= np.float32(prm.near_plane_distance)) & (dep <= np.float32(prm.far_plane_distance))     # the feature gather's planes
        return xy[keep], de[keep], None, dep[keep]
    L, R = world.render_stereo(f)
    xy, _, de, _ = oracle_lib.compute_features(L, prm)
    xyr, _, der, _ = oracle_lib.compute_features(R, prm)
    return xy, de, (xyr, der), None


def _q_to_R(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("kind", sorted(SCENARIOS))
def test_relocalises_after_a_blackout(oracle_lib, kind):
    world, prm, sensor, orc, f = blackout_case(oracle_lib, kind)
    xyz, _, _, desc = orc.map()
    q_last, p_last = orc.pose()
    xy, de, right, dep = frame_features(oracle_lib, world, prm, sensor, f)
    min_inliers = SCENARIOS[kind][2]
    out = RU.relocalise(prm, sensor, xyz, desc, xy, de, right=right, depth=dep, cfg={"min_inliers": min_inliers}, pnp=oracle_lib.pnp)
    Rg, tg = world.pose(f)

    def proj(R, t):
        pc = (xyz - t) @ R
        return np.column_stack([prm.fx * pc[:, 0] / pc[:, 2] + prm.cx, prm.fy * pc[:, 1] / pc[:, 2] + prm.cy]), pc[:, 2]
    (a, za), (b, zb) = proj(_q_to_R(q_last), p_last), proj(Rg, tg)
    front = (za > 0) & (zb > 0)
    far = float((np.linalg.norm(a - b, axis=1)[front] > 2 * prm.tracking_radius).mean())
    err = float(np.linalg.norm(out["p"] - tg))
    print(kind, "frame", f, "map", len(xyz), "features", len(xy), "matched", out["n_matched"], "corr", out["n_corr"], "with point", out["n_with_point"],
          "best", out["best_hypothesis"], out["n_hyp_inliers"], "refined", out["n_refined_inliers"], "error", err, "far", far)
    need = max(min_inliers, prm.min_num_matches_for_tracking)
    assert out["status"] == 0 and out["n_refined_inliers"] >= 2 * need
    assert err < 0.1                                # tests/test_oracle_sequence.py's bound for half-size images
    assert far > 0.5                                # most of the map is out of the frame path's reach: otherwise the case proves nothing
    st = RU.committed_state(out["q"], out["p"], out["n_refined_inliers"])
    assert st["state"] == 2 and st["last_matches"] == (out["n_refined_inliers"],) * 3 and not st["mm_lin_vel"].any() and st["mm_ang_vel"].tolist() == [1, 0, 0, 0]


# ---- the binding ----------------------------------------------------------------------------------------------------------------------------------
def test_record_sizes_and_defaults_of_the_binding():
    assert ctypes.sizeof(lvt_amd.RelocConfig) == lvt_amd.RELOC_CONFIG_SIZE == 32
    assert ctypes.sizeof(lvt_amd.RelocResult) == lvt_amd.RELOC_RESULT_SIZE == 192
    c = lvt_amd.RelocConfig()
    assert (c.n_hypotheses, c.gate_px2, c.min_disparity, c.min_inliers, c.seed, c.dry_run) == (256, 16.0, 1.0, 30, 0, 0)
    assert {k: getattr(c, k) for k in RU.DEFAULTS} == RU.DEFAULTS
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lvt_amd_ext.h")).read()
    assert "#define LVT_AMD_RELOC_CONFIG_SIZE 32" in hdr and "#define LVT_AMD_RELOC_RESULT_SIZE 192" in hdr
    assert lvt_amd.RelocResult._q.offset == 40 and lvt_amd.RelocResult._t.offset == 168 and lvt_amd.RelocConfig.seed.offset == 16


def test_default_config_and_refusals_without_a_device(hip_lib):
    """host code: the library's own defaults, the slice length, and refusals that are decided before the device is touched"""
    c = hip_lib.reloc_default_config()
    assert (c.n_hypotheses, c.gate_px2, c.min_disparity, c.min_inliers, c.seed, c.dry_run) == (256, 16.0, 1.0, 30, 0, 0)
    assert [hip_lib.reloc_slice_length(m) for m in (0, 1, 844, 1024, 1025, 2048, 2049, 32768)] == [32, 32, 32, 32, 64, 64, 96, 1024]
    prm = lvt_amd.kitti_params()
    z3, z2 = np.zeros((4, 3)), np.zeros((4, 2), np.float32)
    for field, value, word in (("n_hypotheses", 0, "n_hypotheses"), ("n_hypotheses", 1025, "n_hypotheses"), ("gate_px2", 0.0, "gate_px2"),
                               ("gate_px2", float("nan"), "gate_px2"), ("min_disparity", float("inf"), "min_disparity"), ("min_inliers", 2, "min_inliers")):
        cfg = lvt_amd.RelocConfig(**{field: value})
        with pytest.raises(ValueError) as e:
            hip_lib.reloc_solve(prm, z3, z2, z3, np.ones(4, bool), cfg)
        assert word in str(e.value) and str(e.value).endswith("(nothing was changed)"), str(e.value)


# ---- the odometry accumulator's policy (lvt_amd_odometry_set_relocalisation), host code: a stub tracker pointer of NULL ------------------------------------
def _script(n=20, lost=(6, 7, 12, 13, 14, 15)):
    """(R, t, status, stamp) of a recorded sequence: a smooth trajectory whose frames `lost` come back LOST with the last tracked pose, as the tracker returns them"""
    from test_odometry import _trajectory
    out, last = [], None
    for i, (R, t) in enumerate(_trajectory(n, 9)):
        if i in lost:
            out.append((last[0], last[1], 3, 0.1 * i))
        else:
            last = (R, t)
            out.append((R, t, 2, 0.1 * i))
    return out


def _run(od, script):
    return [od.push_pose(*step) for step in script]


def _bytes(results):
    return [None if r is None else (r[0].tobytes(), r[1].tobytes()) for r in results]


def test_odometry_policy_unset_is_todays_behaviour(hip_lib):
    """never set, and set and turned off again: the same bytes out of push_pose on a recorded sequence with LOST frames, and the node's arithmetic"""
    from test_odometry import NodeModel, _same_rotation
    script = _script()
    for reset_pose in (True, False):
        plain = _run(hip_lib.Odometry(None, None, reset_pose), script)
        od = hip_lib.Odometry(None, None, reset_pose)
        assert od.set_relocalisation(max_lost_frames=3) == 0 and od.set_relocalisation(max_lost_frames=0) == 0
        assert _bytes(_run(od, script)) == _bytes(plain)
        ref = NodeModel(None, reset_pose)
        for step, got in zip(script, plain):
            exp = ref.push(*step)
            assert (got is None) == (exp is None) == (step[2] == 3)
            if got is not None:
                assert np.allclose(got[0][:3], exp[0][:3], atol=1e-9) and _same_rotation(got[0][3:], exp[0][3:]) and np.allclose(got[1], exp[1], atol=1e-9)


def test_odometry_policy_keeps_the_trajectory_across_a_gap_and_falls_back_to_reset(hip_lib):
    """max_lost_frames = 3, no tracker to relocalise (every attempt fails).  Frames 6, 7 are LOST: nothing is published and nothing is reset, so frame 8's
    delta spans the gap -- the published poses from frame 8 on equal those of an accumulator that simply never saw frames 6 and 7.  Frames 12 .. 15 are
    LOST: the third failure in a row (frame 14) is the reference's reset, and the count starts again at frame 15."""
    from test_odometry import NodeModel, _same_rotation, _trajectory
    script = _script()
    od = hip_lib.Odometry(None, None, True)
    assert od.set_relocalisation(hip_lib.RelocConfig(n_hypotheses=64), max_lost_frames=3) == 0
    got = _run(od, script)
    assert [r is None for r in got] == [s[2] == 3 for s in script]
    skipping = hip_lib.Odometry(None, None, True)                 # the same frames without the LOST ones of the first gap
    for i, step in enumerate(script[:12]):
        if step[2] == 3:
            continue
        exp = skipping.push_pose(*step)
        assert exp[0].tobytes() == got[i][0].tobytes(), i          # the pose is continuous across the gap, to the last bit
        if i == 8:                                                 # ... and the published delta spans it: three frame times
            one = np.linalg.norm(got[5][0][:3] - got[4][0][:3])
            assert 2.0 * one < np.linalg.norm(got[8][0][:3] - got[5][0][:3]) < 4.5 * one
            assert np.allclose(got[8][1][:3], (got[8][0][:3] - got[5][0][:3]) / 0.3, atol=0.2)          # the twist is over the gap's time (odom axes ~ base axes here)
    # the fall-back, against the node's arithmetic with the policy written out: after the third failure in a row (frame 14) the accumulator is the
    # reference's after a reset.  A reset tracker starts again at the identity, so the script's last frames do: with the reset the published poses restart
    # near the origin, without it (max_lost_frames = 5) they would be the old trajectory's end times a meaningless delta
    class PolicyModel(NodeModel):
        def __init__(self, max_lost):
            super().__init__(None, True)
            self.max_lost, self.run = max_lost, 0

        def push(self, R, t, status, stamp):
            if status != 3:
                self.run = 0
            elif self.max_lost > 0:
                self.run += 1
                if self.run < self.max_lost:
                    return None
                self.run = 0
            return super().push(R, t, status, stamp)
    restarted = script[:16] + [(R, t, 2, 0.1 * (16 + i)) for i, (R, t) in enumerate(_trajectory(4, 3))]
    od3, od5 = hip_lib.Odometry(None, None, True), hip_lib.Odometry(None, None, True)
    od3.set_relocalisation(max_lost_frames=3), od5.set_relocalisation(max_lost_frames=5)
    m3, m5 = PolicyModel(3), PolicyModel(5)
    jump = {}
    for i, step in enumerate(restarted):
        for od_, m in ((od3, m3), (od5, m5)):
            g, e = od_.push_pose(*step), m.push(*step)
            assert (g is None) == (e is None), i
            if g is not None:
                assert np.allclose(g[0][:3], e[0][:3], atol=1e-9) and _same_rotation(g[0][3:], e[0][3:]) and np.allclose(g[1], e[1], atol=1e-8), i
                if i == 16:
                    jump[m.max_lost] = float(np.linalg.norm(g[1][:3]))
    # (the accumulated pose telescopes to the last pose pushed whether or not there was a reset; the delta published for frame 16 tells the two apart: one
    #  frame's motion from the origin over 0.5 s against the jump back from the old trajectory's end)
    assert jump[3] < 3.0 < 10.0 < jump[5], jump
    # two failures only (max_lost_frames = 5 would not reset either gap): the whole trajectory is the LOST-free one
    od5 = hip_lib.Odometry(None, None, True)
    od5.set_relocalisation(max_lost_frames=5)
    clean = hip_lib.Odometry(None, None, True)
    last = [od5.push_pose(*s) for s in script][-1]
    for s in script:
        if s[2] == 2:
            exp = clean.push_pose(*s)
    assert last[0].tobytes() == exp[0].tobytes()
    with pytest.raises(ValueError, match="gate_px2.*nothing was changed"):
        od.set_relocalisation(gate_px2=-1.0)
    with pytest.raises(ValueError, match="dry_run.*nothing was changed"):     # the accumulator's relocalisation commits
        od.set_relocalisation(dry_run=1)
    with pytest.raises(TypeError):
        od.set_relocalisation(hip_lib.RelocConfig(), 3, seed=1)


# ---- the correspondence stage's planted cases (tests/reloc_cases.py): each still has the property it is named for ------------------------------------------
def _reloc_case_names():
    import reloc_cases
    return reloc_cases.CASE_NAMES


@pytest.mark.parametrize("name", _reloc_case_names())
def test_correspondence_case_has_its_property(name):
    """with the restatement alone (global_match, correspondences, camera_points_stereo / _rgbd): the counts cross the block boundaries they are meant to
    cross, both outcomes of every planted decision are present, the planted partner is the one the definition picks.  A case that has lost its property
    fails here instead of passing vacuously on the GPU."""
    import reloc_cases
    case, ref = reloc_cases.case_and_answer(name)
    print(name, "--", case["plants"], "| N", ref["n_features"], "M", ref["n_map"], "matched", ref["n_matched"], "corr", ref["n_corr"], "with point", ref["n_with_point"])
    assert case["plants"] and ref["n_features"] <= RU.NF_MAX and ref["n_map"] <= RU.MAP_MAX
    case["check"](case, ref)


def test_correspondence_cases_cover_the_issue_list():
    import reloc_cases
    got = {n: reloc_cases.case_and_answer(n) for n in reloc_cases.CASE_NAMES}
    sizes = {(r["n_features"], r["n_map"]) for n, (_, r) in got.items() if n.startswith("A-")}
    assert {(n, 3300) for n in (0, 1, 1023, 1024, 1025, 2049, 4096)} | {(1025, m) for m in (0, 1, 2, 33)} | {(4096, 32768)} == sizes
    assert max(r["n_corr"] for _, r in got.values()) > 2048 and max(r["n_with_point"] for _, r in got.values()) > 2048
    assert {c["sensor"] for c, _ in got.values()} == {1, 2} and {c["map_copy"] for c, _ in got.values()} == {0, 1} and any(c["lost_frame"] for c, _ in got.values())
    assert sorted(r["n_features"] for n, (_, r) in got.items() if n.startswith("F-")) == [1025, 4096]


def _correspond(hip_lib, case):
    return hip_lib.reloc_correspond(case["prm"], case["sensor"], case["xy_l"], case["desc_l"], case["map_xyz"], case["map_desc"], right=case["right"],
                                    depth=case["depth"], other=case["other"], map_copy=case["map_copy"], lost_frame=case["lost_frame"],
                                    cfg=lvt_amd.RelocConfig(min_disparity=case["min_disparity"]))


def test_correspond_refusals_without_a_device(hip_lib):
    """host code: every refusal of lvt_amd_reloc_correspond is decided before the device is touched"""
    import dataclasses
    import reloc_cases
    case, _ = reloc_cases.case_and_answer("A-N1-M3300")
    for change, word in ((dict(sensor=3), "sensor"), (dict(map_copy=2), "map_copy"), (dict(lost_frame=-1), "lost_frame"), (dict(min_disparity=0.0), "min_disparity"),
                         (dict(sensor=2), "NULL"), (dict(prm=dataclasses.replace(case["prm"], img_height=0)), "parameters")):
        with pytest.raises(ValueError) as e:
            _correspond(hip_lib, dict(case, **change))
        assert word in str(e.value) and str(e.value).startswith("lvt_amd_reloc_correspond: ") and str(e.value).endswith("(nothing was changed)"), str(e.value)
    big = np.zeros((4097, 2), np.float32)
    with pytest.raises(ValueError, match="4096.*nothing was changed"):
        _correspond(hip_lib, dict(case, xy_l=big, desc_l=np.zeros((4097, 32), np.uint8)))
