"""The HIP path through turns past 180 degrees (TURN_CASES, case_tables.py; the worlds are turn_worlds.py), held to the oracle: the w >= 0 flip of the
published pose inside the pipeline, motion_predict's d < 0 arm and the w < 0 prediction it hands to the next k_pnp, map points behind the camera in front
of is_point_visible, rotation matrices far from the identity -- and the motion model alone on MOTION_EDGE_CASES.  test_case_tables.py asserts with the
oracle alone that the cases take these branches; profiles/turns.md records what was measured."""
import ctypes

import numpy as np
import pytest

from case_tables import MOTION_EDGE_CASES, TURN_CASES, TURN_KEEP_FRAMES, TURN_KEEP_POINTS, behind_camera_in_image, turn_case
from parity_util import POSE_TOL, PRED_TOL, diff_frame, pose_errors, run_sequence

pytestmark = pytest.mark.gpu

STEREO_TURNS = [n for n in TURN_CASES if TURN_CASES[n][4] == 1]
LISTS = [("0", "wave_per_query_lists"), ("1", "binned_list_kernel")]


def _sequence_with_signed_poses(name, monkeypatch, binned):
    """run_sequence (diff_frame on every frame) plus, on every frame, the pose quaternion and position compared SIGN-SENSITIVELY (pose_errors compares rotation
    matrices: q and -q are one matrix); for room_loop_keep the behind-the-camera count of the guard on the HIP side's own map and predicted pose"""
    monkeypatch.setenv("LVT_AMD_BINNED_LISTS", binned)
    world, prm, sensor, n = turn_case(name)
    worst = dict(q=0.0, p=0.0, pred_q=0.0, pred_p=0.0)
    signed, behind, at_match = [], [], [np.zeros((0, 3))]

    def on_frame(i, hip, orc):
        (qh, ph), (qo, po) = hip.pose(), orc.pose()
        eq, ep = float(np.abs(qh - qo).max()), float(np.abs(ph - po).max())
        worst["q"], worst["p"] = max(worst["q"], eq), max(worst["p"], ep)
        if eq > PRED_TOL or ep > PRED_TOL:
            signed.append(f"frame {i}: pose q hip={qh} oracle={qo} (|dq| {eq:.3e}, |dp| {ep:.3e})")
        if hip.counts()["map_size_at_match"] > 0:
            (qh, ph), (qo, po) = hip.predicted_pose(), orc.predicted_pose()
            worst["pred_q"], worst["pred_p"] = max(worst["pred_q"], float(np.abs(qh - qo).max())), max(worst["pred_p"], float(np.abs(ph - po).max()))
            if name == "room_loop_keep":
                assert len(at_match[0]) == hip.counts()["map_size_at_match"]
                behind.append(behind_camera_in_image(prm, at_match[0], qh, ph))
        if name == "room_loop_keep":
            at_match[0] = hip.map()[0]
    res, hip, orc = run_sequence(world, prm, sensor, range(n), on_frame=on_frame)
    bad = [(i, m) for i, m, _, _ in res if m]
    print(f"{name} lists={binned}: max |dq| {worst['q']:.3e} |dp| {worst['p']:.3e} predicted |dq| {worst['pred_q']:.3e} |dp| {worst['pred_p']:.3e} "
          f"e_t {max(r[2] for r in res):.3e} e_R {max(r[3] for r in res):.3e}")
    assert not bad, f"{name}: first divergence at frame {bad[0][0]}: {bad[0][1][:6]}"
    assert not signed, signed[:4]
    assert hip.get_state() == orc.status == 2 and hip.last_error() == ""
    return behind


@pytest.mark.parametrize("binned,_id", LISTS, ids=[x[1] for x in LISTS])
@pytest.mark.parametrize("name", STEREO_TURNS)
def test_turn_case_equals_the_oracle(hip_lib, oracle_lib, monkeypatch, name, binned, _id):
    behind = _sequence_with_signed_poses(name, monkeypatch, binned)
    if name == "room_loop_keep":
        behind = np.array(behind)
        print(f"room_loop_keep (HIP map, HIP prediction): {int((behind >= TURN_KEEP_POINTS).sum())} frames with {TURN_KEEP_POINTS}+ points, peak {behind.max()}")
        assert (behind >= TURN_KEEP_POINTS).sum() >= TURN_KEEP_FRAMES


@pytest.mark.parametrize("binned,_id", LISTS, ids=[x[1] for x in LISTS])
def test_rgbd_room_equals_the_oracle(hip_lib, oracle_lib, monkeypatch, binned, _id):
    """room_rgbd through lvt_amd_track_rgbd: the same turn seen by the RGB-D branch of the gather and of the triangulation"""
    assert TURN_CASES["room_rgbd"][4] == 2
    _sequence_with_signed_poses("room_rgbd", monkeypatch, binned)


def _wait_pose(hip_lib, hip):
    """lvt_amd_wait_pose: (q, p, state) of the oldest un-collected frame -- the pose as the tracker holds it, sign included"""
    q, p = np.zeros(4), np.zeros(3)
    fn = hip_lib.load_library().lvt_amd_wait_pose
    fn.restype = ctypes.c_int
    st = fn(ctypes.c_void_p(hip._h), q.ctypes.data_as(ctypes.c_void_p), p.ctypes.data_as(ctypes.c_void_p))
    return q, p, st


@pytest.mark.parametrize("name", ["roll_past_180", "room_loop_keep"])
def test_turn_case_through_the_async_path(hip_lib, oracle_lib, name):
    """lvt_amd_track_async, three frames in flight: the early stream of frame t + 1 starts from the flipped pose of frame t.  Every frame's pose (signed
    quaternion and position within PRED_TOL) and state against the oracle's, the full frame diff at the end."""
    from oracle import pyoracle as O
    world, prm, sensor, n = turn_case(name)
    hip = hip_lib.LvtSystem.create(prm, 1)
    orc = O.Oracle(prm, 1)
    frames = [world.render_stereo(i) for i in range(n)]
    got, inflight = [], 0
    for a, b in frames:
        assert hip.track_async(a, b) == 0
        inflight += 1
        if inflight >= 3:
            got.append(_wait_pose(hip_lib, hip)); inflight -= 1
    while inflight:
        got.append(_wait_pose(hip_lib, hip)); inflight -= 1
    worst = 0.0
    for i, (a, b) in enumerate(frames):
        orc.track(a, b)
        qo, po = orc.pose()
        qh, ph, st = got[i]
        e = max(float(np.abs(qh - qo).max()), float(np.abs(ph - po).max()))
        worst = max(worst, e)
        assert e <= PRED_TOL and st == orc.status == 2, f"frame {i}: hip q {qh} p {ph} state {st}; oracle q {qo} p {po} state {orc.status}"
    print(f"{name} async: max signed pose difference {worst:.3e}")
    msgs = diff_frame(hip, orc)
    assert not msgs, msgs[:6]
    assert hip.last_error() == ""


def test_turn_cases_in_one_lockstep_batch(hip_lib, oracle_lib):
    """one mixed lock-step batch of roll_past_180 (76 frames), room_loop and room_loop_keep (150): k_hamming_batched_lists<MAP>'s own prologue (its
    motion_predict) and visibility test.  The shorter sequence is absent after its last frame.  Every pose and state and each sequence's counters against
    its own oracle."""
    from test_gpu_mixed_batch import Seq, check_against_own_oracles, run
    seqs = []
    for name in STEREO_TURNS:
        world, prm, _, n = turn_case(name)
        seqs.append(Seq(world, prm, n))
    steps = max(q.n for q in seqs)
    assert min(q.n for q in seqs) < steps
    schedule = [[i if i < q.n else None for q in seqs] for i in range(steps)]
    batch = hip_lib.LvtBatch.create_mixed([q.prm for q in seqs])
    got = run(batch, seqs, schedule)
    assert batch.last_error() == "", batch.last_error()
    check_against_own_oracles(batch, seqs, schedule, got)


def test_motion_model_on_the_device_equals_the_oracle(hip_lib, oracle_lib):
    """lvt_amd_motion_predict (one device thread through the frame path's motion_predict) on MOTION_EDGE_CASES against the oracle, which
    test_oracle_motion_model_equals_the_longdouble_restatement pins.  Bit-identical inputs; -ffp-contract=off on both sides.
      p_out, next[8..13], next[0..3]: add, subtract, multiply by 0.5 or copies -- bit-equal.
      q_out, next[4..7]: about 20 roundings on quantities <= 1 plus the device's acos / sin within a rounding or two of the host's: a few 1e-15; the bound
      is 1e-13 absolute (profiles/turns.md records the largest difference observed)."""
    worst, worst_at = 0.0, ""
    for lab, st, q, p in MOTION_EDGE_CASES:
        no, qo, po = oracle_lib.motion_predict(st, q, p)
        nh, qh, ph = hip_lib.motion_predict(st, q, p)
        assert ph.tobytes() == po.tobytes() and nh[8:14].tobytes() == no[8:14].tobytes() and nh[0:4].tobytes() == no[0:4].tobytes(), \
            f"{lab}: hip p {ph} next {nh}; oracle p {po} next {no}"
        e = max(float(np.abs(qh - qo).max()), float(np.abs(nh[4:8] - no[4:8]).max()))
        if not e <= worst:
            worst, worst_at = e, lab
        assert e <= 1e-13, f"{lab}: quaternions differ by {e:.3e}: hip q {qh} ang_vel {nh[4:8]}; oracle q {qo} ang_vel {no[4:8]}"
    print(f"motion model, device vs oracle: largest quaternion difference {worst:.3e} ({worst_at})")
