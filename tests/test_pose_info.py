"""Pose uncertainty, CPU tier: the reference's Jacobian against central differences of the projection, lvt_amd_pose_info_to_ros, the covariance the
odometry accumulator publishes against central differences of the accumulator itself, and the record's size.  Host code only: no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import lvt_amd
import pose_info_util as U
from case_tables import intrinsics


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def _random_q(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _spd(rng):
    A = rng.normal(size=(6, 6))
    return A @ A.T + 0.1 * np.eye(6)


@pytest.mark.parametrize("name", ["kitti", "tum"])
def test_reference_jacobian_equals_central_differences(name):
    """J of pose_info_util.reference against (e(xi + h e_k) - e(xi - h e_k)) / 2h, h = 1e-6, on 50 random edges: |dJ| <= 1e-5 max|J|"""
    prm = intrinsics(name)
    rng = np.random.default_rng(7)
    q = _random_q(rng)
    R, p = U.quat_to_R(q), rng.normal(0, 0.5, 3)
    pc = np.column_stack([rng.uniform(-8, 8, 50), rng.uniform(-3, 3, 50), rng.uniform(4, 40, 50)])
    X = pc @ R.T + p
    J = U.jacobians(prm, R, U.project(prm, R, p, X)[1])
    h = 1e-6
    for k in range(6):
        d = np.zeros(6); d[k] = h
        up = U.project(prm, R @ U.exp_so3(d[3:]), p + d[:3], X)[0]
        dn = U.project(prm, R @ U.exp_so3(-d[3:]), p - d[:3], X)[0]
        fd = (up - dn) / (2 * h)          # (the observation is a constant of e)
        assert np.abs(fd - J[:, :, k]).max() <= 1e-5 * np.abs(J).max(), (k, np.abs(fd - J[:, :, k]).max(), np.abs(J).max())


def test_to_ros_rotates_the_angular_block_onto_world_axes():
    rng = np.random.default_rng(11)
    for trial in range(20):
        S = _spd(rng)
        q = _random_q(rng)
        if trial % 2:
            q = -q if q[0] > 0 else q          # w of either sign
        else:
            q = q if q[0] > 0 else -q
        R = U.quat_to_R(q)
        M = np.eye(6); M[3:, 3:] = R
        want = M @ S @ M.T
        got = lvt_amd.pose_info_to_ros(S, R)
        assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max(), np.abs(got - want).max()
        assert np.array_equal(got, got.T)


def _trajectory(n, seed):
    rng = np.random.default_rng(seed)
    R, t = np.eye(3), np.zeros(3)
    out = []
    for i in range(n):
        R = R @ _rot("y", rng.normal(0, 0.02)) @ _rot("x", rng.normal(0, 0.005)) @ _rot("z", rng.normal(0, 0.005))
        t = t + R @ np.array([rng.normal(0, 0.02), rng.normal(0, 0.01), 0.8 + rng.normal(0, 0.05)])
        out.append((R.copy(), t.copy()))
    return out


def _quat_xyzw_to_R(q):
    return U.quat_to_R([q[3], q[0], q[1], q[2]])


def _replay(traj, b2s, lost_at, last_R, last_t):
    """a fresh accumulator fed the trajectory with its last pose replaced; the pose it publishes for that last frame as (R_ob, p_ob)"""
    od = lvt_amd.Odometry(None, b2s, True)
    out = None
    for i, (R, t) in enumerate(traj):
        last = i == len(traj) - 1
        out = od.push_pose(last_R if last else R, last_t if last else t, 3 if i == lost_at else 2, 0.1 * i)
    od.close()
    return _quat_xyzw_to_R(out[0][3:]), out[0][:3].copy()


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("lost_at", [None, 14])
def test_odometry_covariance_equals_the_accumulators_own_differences(with_base, lost_at):
    """cov_out against M S M^T with M the central differences (h = 1e-5) of the published pose under a perturbation of the LAST pushed pose in the record's
    convention (position on world axes, rotation R Exp([dtheta]x)), the rotation difference read from R' R^T: within 1e-7 max|M S M^T| (truncation h^2 = 1e-10,
    rounding eps / h ~ 2e-11: three orders left).  Pose and twist are bit-identical to push_pose's."""
    b2s = None
    if with_base:
        b2s = np.eye(4); b2s[:3, :3] = _rot("z", 0.3) @ _rot("y", -0.2); b2s[:3, 3] = [0.4, -0.1, 1.2]
        b2s = b2s[:3, :]
    traj = _trajectory(30, 3 + (1 if with_base else 0))
    S = _spd(np.random.default_rng(5)) * 1e-6
    plain, withcov = lvt_amd.Odometry(None, b2s, True), lvt_amd.Odometry(None, b2s, True)
    got = None
    for i, (R, t) in enumerate(traj):
        status = 3 if i == lost_at else 2
        a = plain.push_pose(R, t, status, 0.1 * i)
        b = withcov.push_pose_cov(R, t, status, 0.1 * i, S)
        assert (a is None) == (b is None) == (i == lost_at)
        if a is not None:
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), i
            got = b[2]
    R_last, t_last = traj[-1]
    R0, p0 = _replay(traj, b2s, lost_at, R_last, t_last)
    h = 1e-5
    M = np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6); d[k] = h
        Ru, pu = _replay(traj, b2s, lost_at, R_last @ U.exp_so3(d[3:]), t_last + d[:3])
        Rd, pd = _replay(traj, b2s, lost_at, R_last @ U.exp_so3(-d[3:]), t_last - d[:3])
        M[:3, k] = (pu - pd) / (2 * h)
        M[3:, k] = (U.log_so3(Ru @ R0.T) - U.log_so3(Rd @ R0.T)) / (2 * h)
    want = M @ S @ M.T
    assert np.abs(got - want).max() <= 1e-7 * np.abs(want).max(), (np.abs(got - want).max(), np.abs(want).max())
    assert np.array_equal(got, got.T)
    if with_base:    # the lever arm of base_to_sensor couples rotation into position: the block is not just a rotated copy
        Mrot = np.zeros((6, 6)); Mrot[:3, :3] = M[:3, :3]; Mrot[3:, 3:] = M[3:, 3:]
        assert np.abs(Mrot @ S @ Mrot.T - want).max() > 1e-3 * np.abs(want).max()


def test_odometry_covariance_is_zero_without_a_valid_input():
    traj = _trajectory(6, 9)
    od = lvt_amd.Odometry()
    S = _spd(np.random.default_rng(1))
    for i, (R, t) in enumerate(traj[:3]):
        out = od.push_pose_cov(R, t, 2, 0.1 * i, None)          # no covariance handed in (what update_cov does for a record whose status is not 1)
        assert out is not None and not out[2].any()
    out = od.push_pose_cov(*traj[3], 2, 0.3, S)
    assert out is not None and out[2].any()
    # LOST and a stale stamp publish nothing: the output array is still zeroed
    L = lvt_amd.load_library()
    cov = np.full(36, 7.0); R = np.ascontiguousarray(traj[4][0]); t = np.ascontiguousarray(traj[4][1]); Sf = np.ascontiguousarray(S).reshape(36)
    vp = ctypes.c_void_p
    assert L.lvt_amd_odometry_push_pose_cov(vp(od._h), lvt_amd._p(R), lvt_amd._p(t), 2, 0.05, lvt_amd._p(Sf), None, None, lvt_amd._p(cov)) == 0 and not cov.any()
    cov[:] = 7.0
    assert L.lvt_amd_odometry_push_pose_cov(vp(od._h), lvt_amd._p(R), lvt_amd._p(t), 3, 0.5, lvt_amd._p(Sf), None, None, lvt_amd._p(cov)) == 0 and not cov.any()
    assert L.lvt_amd_odometry_push_pose_cov(vp(od._h), None, None, 2, 0.6, None, None, None, None) == -1
    assert L.lvt_amd_odometry_update_cov(vp(od._h), None, None, 1, 1, 0.0, None, None, None) == -1   # no tracker attached


def test_record_size_is_the_same_in_c_and_python():
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "lvt_amd_ext.h")).read()
    m = re.search(r"#define LVT_AMD_POSE_INFO_SIZE (\d+)", hdr)
    assert m and int(m.group(1)) == ctypes.sizeof(lvt_amd.PoseInfo) == lvt_amd.POSE_INFO_SIZE == 616
    assert "static_assert(sizeof(lvt_amd_pose_info) == LVT_AMD_POSE_INFO_SIZE" in hdr
    # the layout the header declares: two 6 x 6 matrices, two sums, six ints
    f = dict((n, (getattr(lvt_amd.PoseInfo, n).offset, getattr(lvt_amd.PoseInfo, n).size)) for n, _ in lvt_amd.PoseInfo._fields_)
    assert f["_cov"] == (0, 288) and f["_info"] == (288, 288) and f["chi2"] == (576, 8) and f["sq_err"] == (584, 8)
    assert [f[n][0] for n in ("n_edges", "n_inliers", "n_borderline", "status", "frame", "reserved")] == [592, 596, 600, 604, 608, 612]
    # the library was compiled against that header: a zero-length evaluation is refused without a device only for bad arguments
    L = lvt_amd.load_library()
    assert L.lvt_amd_pose_info_eval(None, None, None, None, None, 0, None) == -1
    rec = lvt_amd.PoseInfo()
    assert L.lvt_amd_get_pose_info(None, 0, ctypes.byref(rec)) == -1 and L.lvt_amd_enable_pose_info(None, 1) == -1
