"""Pose uncertainty on the GPU (k_pose_info, lvt_amd_enable_pose_info / lvt_amd_get_pose_info / lvt_amd_pose_info_eval): the stand-alone evaluation and
the per-frame records of solo handles, frames in flight, lock-step batches, LOST, snapshots -- held to pose_info_util.reference, a numpy restatement of
the definition in include/lvt_amd_ext.h, at the bounds that definition's arithmetic supports:
  |dinfo_ij| <= 1e-10 sqrt(info_ii info_jj)   (e carries ~1e-12 px at u ~ 10^3 px in fp64, w follows by 2 |e| w / 5.991 of that, J a few ulp: two orders left)
  max |info cov - I| <= 1e-9 on the device's own two matrices, rows / columns scaled by sqrt(diag);  |dcov_ij| <= 1e-9 sqrt(cov_ii cov_jj) against inv(device info)
  counts exact wherever the reference finds no edge within 1e-6 of the gate."""
import ctypes
import os

import numpy as np
import pytest

import pose_info_util as U
from case_tables import intrinsics, pnp_case
from parity_util import make_case

pytestmark = pytest.mark.gpu

EVAL_SIZES = [0, 1, 2, 3, 5, 6, 7, 63, 64, 65, 255, 256, 257, 513, 4096]


def _axis_q(axis, deg):
    a = np.deg2rad(deg) / 2
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.array([np.cos(a), *(np.sin(a) * ax)])


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def eval_case(name, n):
    """pnp_case's edges and a pose a few cm / a tenth of a degree off its truth: the errors straddle the 5.991 gate.  pnp_case keeps its truth to
    itself; it is drawn again here from the same seed (points, then angles, then position) and CHECKED against the observations it produced."""
    prm = intrinsics(name)
    X, uv = pnp_case(np.random.default_rng(4000 + n), prm, n)
    rng = np.random.default_rng(4000 + n)
    for _ in range(3):
        rng.uniform(0, 1, n)
    ang = rng.normal(0, 0.01, 3)
    q_true = np.array([1.0, *(ang / 2)]); q_true /= np.linalg.norm(q_true)
    p_true = rng.normal(0, 0.3, 3)
    clean = np.arange(n) % 9 != 0          # (every ninth observation is a 25-px outlier)
    if clean.any():
        e = U.project(prm, U.quat_to_R(q_true), p_true, X)[0] - uv
        assert np.median(np.abs(e[clean])) < 1.0, "case_tables.pnp_case no longer draws its truth this way"
    q = _qmul(q_true, _axis_q((0.3, 1.0, -0.2), 0.1)); q /= np.linalg.norm(q)
    return prm, X, uv, q, p_true + np.array([0.02, -0.01, 0.02])


def compare(rec, ref, what):
    """any record of an evaluation against the reference: valid ones at the bounds, degenerate ones with info delivered and cov zero"""
    U.check_counts(rec, ref, what)
    assert rec.status == ref["status"], (what, rec.status, ref["status"], rec.n_inliers)
    if rec.status == 1:
        return U.check_valid(rec, ref, what)
    assert not rec.cov.any(), what
    assert np.array_equal(rec.info, rec.info.T)
    assert U.info_error(rec.info, ref["info"]) <= U.INFO_TOL if ref["info"].any() else not rec.info.any(), what
    return None


@pytest.mark.parametrize("name", ["kitti", "tum"])
def test_eval_against_the_reference_over_edge_counts(hip_lib, name):
    worst = np.zeros(3)
    seen = set()
    for n in EVAL_SIZES:
        prm, X, uv, q, p = eval_case(name, n)
        ref = U.reference(prm, q, p, X, uv)
        rec = hip_lib.pose_info_eval(prm, q, p, X, uv)
        got = compare(rec, ref, f"{name} n={n}: inliers {rec.n_inliers} status {rec.status}")
        seen.add(rec.status)
        if got:
            worst = np.maximum(worst, got)
        if n >= 63:       # the errors straddle the gate: both sides are populated
            assert ref["status"] == 1 and 0.2 * n < ref["n_inliers"] < 0.95 * n, (n, ref["n_inliers"])
    print(f"{name}: observed maxima info {worst[0]:.2e} identity {worst[1]:.2e} cov {worst[2]:.2e}")
    assert seen == {1, 2}


def planted(prm, rng, n=40):
    """n well-spread edges with errors of ~1 px at a pose with w < 0, to which the planted ones are appended"""
    q = -_axis_q((0.2, -1.0, 0.4), 25.0)
    assert q[0] < 0
    R, p = U.quat_to_R(q), np.array([0.4, -0.3, 1.1])
    pc = np.column_stack([rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), rng.uniform(5, 40, n)])
    X = pc @ R.T + p
    uv = (U.project(prm, R, p, X)[0] + rng.normal(0, 0.7, (n, 2))).astype(np.float32)
    return q, R, p, X, uv


@pytest.mark.parametrize("name", ["kitti", "tum"])
def test_eval_planted_edges(hip_lib, name):
    prm = intrinsics(name)
    rng = np.random.default_rng(21)
    q, R, p, X0, uv0 = planted(prm, rng)
    base = U.reference(prm, q, p, X0, uv0)
    assert base["status"] == 1 and not base["near"].any()

    def with_edges(Xs, obs):
        X, uv = np.vstack([X0, np.asarray(Xs).reshape(-1, 3)]), np.vstack([uv0, np.asarray(obs, np.float32).reshape(-1, 2)])
        return X, uv, U.reference(prm, q, p, X, uv), hip_lib.pose_info_eval(prm, q, p, X, uv)

    # e.e = 5.991 -+ 1e-3: decided both ways, clear of the borderline margin
    for sign, inlier in ((-1, True), (+1, False)):
        o = np.array([700.25, 210.5], np.float32)
        Xp, e2 = U.point_for(prm, R, p, o, 17.0, U.TH2 + sign * 1e-3, (0.6, -0.8))
        assert abs(e2 - (U.TH2 + sign * 1e-3)) < 1e-9
        X, uv, ref, rec = with_edges([Xp], [o])
        assert bool(ref["inlier"][-1]) is inlier and not ref["near"].any()
        compare(rec, ref, f"{name} gate {sign:+d}e-3")
        assert rec.n_inliers == base["n_inliers"] + (1 if inlier else 0) and rec.n_borderline == 0

    # three edges inside +-1e-7 of the gate: counted, and the matrices accepted with either decision for each
    Xs, obs = [], []
    for k, off in enumerate((-6e-8, 2e-8, 7e-8)):
        o = np.array([300.5 + 150 * k, 120.25 + 40 * k], np.float32)
        Xp, e2 = U.point_for(prm, R, p, o, 9.0 + 6 * k, U.TH2 + off, (1.0, 0.5 - k))
        assert abs(e2 - U.TH2) < 1e-7
        Xs.append(Xp); obs.append(o)
    X, uv, ref, rec = with_edges(Xs, obs)
    assert ref["near"].sum() == 3 and rec.n_borderline == 3 and rec.status == 1
    ok = []
    for mask in range(8):
        info = base["info"].copy()
        for k in range(3):
            if mask >> k & 1:
                i = len(X0) + k
                info += (1.0 / (1.0 + ref["e2"][i] / U.TH2)) * (ref["J"][i].T @ ref["J"][i])
        if U.info_error(rec.info, info) <= U.INFO_TOL:
            ok.append(mask)
    assert len(ok) == 1 and rec.n_inliers == base["n_inliers"] + bin(ok[0]).count("1"), (ok, rec.n_inliers)
    e_ident, e_cov = U.cov_errors(rec.info, rec.cov)
    assert e_ident <= U.IDENT_TOL and e_cov <= U.COV_TOL

    # a point behind the camera that projects ONTO its observation (e = 0, pcz < 0), a NaN coordinate, a 1e5-px outlier
    pcb = np.array([1.5, -0.7, -12.0])
    Xb = R @ pcb + p
    ob = U.project(prm, R, p, Xb)[0][0].astype(np.float32)
    Xn = X0[3].copy(); Xn[1] = np.nan
    Xo = X0[5].copy()
    X, uv, ref, rec = with_edges([Xb, Xn, Xo], [ob, uv0[3], uv0[5] + np.float32(1e5)])
    assert ref["e2"][len(X0)] < 1e-6 and ref["pc"][len(X0), 2] < 0 and np.isnan(ref["e2"][len(X0) + 1]) and ref["e2"][-1] > 1e9
    compare(rec, ref, f"{name} behind / NaN / outlier")
    assert rec.n_inliers == base["n_inliers"] and rec.n_edges == len(X0) + 3
    assert U.info_error(rec.info, base["info"]) <= U.INFO_TOL and np.isfinite(rec.chi2)

    # q of the other sign: the same record, bit for bit
    a, b = hip_lib.pose_info_eval(prm, q, p, X0, uv0), hip_lib.pose_info_eval(prm, -q, p, X0, uv0)
    assert a.to_bytes() == b.to_bytes() and a.status == 1

    # degenerate geometry: all points identical; all on one line through the camera -- status 2, cov zero, info equal to the reference
    Xsame = np.repeat(X0[:1], 12, axis=0)
    osame = np.repeat(U.project(prm, R, p, X0[:1])[0], 12, axis=0).astype(np.float32)
    ray = np.array([0.2, -0.1, 1.0])
    Xline = (np.linspace(4, 30, 12)[:, None] * ray[None, :]) @ R.T + p
    oline = U.project(prm, R, p, Xline)[0].astype(np.float32)
    for what, Xd, od in (("identical", Xsame, osame), ("line", Xline, oline)):
        ref, rec = U.reference(prm, q, p, Xd, od), hip_lib.pose_info_eval(prm, q, p, Xd, od)
        assert ref["n_inliers"] == 12 and ref["status"] == 2, (what, ref["n_inliers"], ref["status"])
        compare(rec, ref, f"{name} {what}")
        assert rec.status == 2 and rec.n_inliers == 12 and not rec.cov.any() and rec.info.any()

    # n_inliers 0 and 2
    for keep in (0, 2):
        uvk = uv0 + np.float32(40.0)
        uvk[:keep] = uv0[:keep]
        ref, rec = U.reference(prm, q, p, X0, uvk), hip_lib.pose_info_eval(prm, q, p, X0, uvk)
        assert ref["n_inliers"] == keep
        compare(rec, ref, f"{name} {keep} inliers")
        assert rec.status == 2 and rec.n_inliers == keep and rec.n_edges == len(X0) and not rec.cov.any()

    # arguments
    L = hip_lib.load_library()
    pod = prm.to_pod()
    out = hip_lib.PoseInfo()
    assert L.lvt_amd_pose_info_eval(ctypes.byref(pod), hip_lib._p(q), hip_lib._p(p), hip_lib._p(X0), hip_lib._p(uv0), 4097, ctypes.byref(out)) == -1
    assert L.lvt_amd_pose_info_eval(ctypes.byref(pod), hip_lib._p(q), hip_lib._p(p), hip_lib._p(X0), hip_lib._p(uv0), -1, ctypes.byref(out)) == -1


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------------------------
PIPE = {"kitti": 14, "tum": 8}     # frames 0 .. n - 1 of make_case(kind), default seeds


def frames_of(kind):
    world, prm, sensor = make_case(kind)
    n = PIPE[kind]
    return prm, sensor, [world.render_stereo(i) if sensor == 1 else world.render_rgbd(i) for i in range(n)]


def snapshot_of(h, R, t, keys=None):
    c = h.counts()
    c.pop("row_fallback", None)       # (how the streams met, not what was computed)
    return {"R": R.copy(), "t": t.copy(), "state": h.get_state(), "counts": c}


@pytest.fixture(scope="module")
def pipe(hip_lib):
    """per kind: a plain handle's frames, then an enabled handle's frames with its records and the reference evaluated from the device's own matches,
    features and pose.  Computed once, read by the tests below."""
    out = {}
    for kind in PIPE:
        prm, sensor, frames = frames_of(kind)
        plain = hip_lib.LvtSystem.create(prm, sensor)
        base = [snapshot_of(plain, *plain.track(*f)) for f in frames]
        assert plain.last_error() == "", plain.last_error()
        plain.close()
        h = hip_lib.LvtSystem.create(prm, sensor)
        assert h.enable_pose_info(True) == 0, h.last_error()
        recs, refs, own = [], [], []
        for f in frames:
            R, t = h.track(*f)
            rec = h.pose_info()
            own.append(snapshot_of(h, R, t))
            recs.append(rec)
            fi, X = h.matches()
            xy = h.features(0)[0]
            q, p = h.pose()
            refs.append(U.reference(prm, q, p, X, xy[fi]) if rec.status else None)
        assert h.last_error() == "", h.last_error()
        h.close()
        out[kind] = {"prm": prm, "sensor": sensor, "frames": frames, "plain": base, "own": own, "recs": recs, "refs": refs}
    return out


@pytest.mark.parametrize("kind", list(PIPE))
def test_pipeline_records_against_the_reference(pipe, kind):
    P = pipe[kind]
    assert P["recs"][0].status == 0 and not P["recs"][0].info.any()
    worst = np.zeros(3)
    for i in range(1, PIPE[kind]):
        rec, ref, c = P["recs"][i], P["refs"][i], P["own"][i]["counts"]
        assert rec.status == 1 and rec.frame == c["frame"], (i, rec.status, rec.frame, c["frame"])
        gap = float(np.nanmin(np.abs(ref["e2"] - U.TH2)))
        print(f"{kind} frame {i}: edges {rec.n_edges} inliers {rec.n_inliers} (solver {c['pnp_inliers']}) nearest edge to the gate {gap:.2e} "
              f"sigma_p max {np.sqrt(np.diag(rec.cov)[:3].max()) * 1e3:.3f} mm chi2 {rec.chi2:.2f}")
        assert not ref["near"].any(), f"{kind} frame {i}: an edge within 1e-6 of the gate ({gap:.2e}): the inputs have changed, this frame no longer decides cleanly"
        assert rec.n_edges == c["n_matches"]
        worst = np.maximum(worst, compare(rec, ref, f"{kind} frame {i}"))
        assert 0 <= rec.n_inliers - c["pnp_inliers"] <= 2, (i, rec.n_inliers, c["pnp_inliers"])
    print(f"{kind}: observed maxima info {worst[0]:.2e} identity {worst[1]:.2e} cov {worst[2]:.2e}")


@pytest.mark.parametrize("kind", list(PIPE))
def test_a_handle_without_pose_info_tracks_bit_identically(pipe, kind):
    P = pipe[kind]
    for i, (a, b) in enumerate(zip(P["plain"], P["own"])):
        assert a["R"].tobytes() == b["R"].tobytes() and a["t"].tobytes() == b["t"].tobytes(), i
        assert a["state"] == b["state"] and a["counts"] == b["counts"], (i, a["counts"], b["counts"])


@pytest.mark.parametrize("kind", list(PIPE))
def test_three_frames_in_flight(hip_lib, pipe, kind):
    """lvt_amd_get_pose_info answers where lvt_amd_get_pose does: for the last frame enqueued, after collecting what is in flight.  Groups of three frames
    go in through track_async with nothing collected in between, the oldest is waited for, then the record is read: it is the group's last frame's, byte for
    byte the synchronous run's.  Three runs whose first group has 1, 2 and 3 frames put every frame at the end of a group once."""
    P = pipe[kind]
    n = PIPE[kind]
    seen = set()
    for first in (1, 2, 3):
        h = hip_lib.LvtSystem.create(P["prm"], P["sensor"])
        assert h.enable_pose_info(True) == 0
        i, size = 0, first
        while i < n:
            hi = min(i + size, n)
            for k in range(i, hi):
                assert h.track_async(*P["frames"][k]) == 0, h.last_error()
            st = h.host_stats()
            assert st["enqueued"] - st["collected"] == hi - i      # all of them in flight (a held frame counts as enqueued)
            h.wait()
            rec = h.pose_info()
            assert rec.to_bytes() == P["recs"][hi - 1].to_bytes(), (first, hi - 1, rec.status, rec.frame)
            assert rec.frame == h.counts()["frame"]
            seen.add(hi - 1)
            i, size = hi, 3
        assert h.last_error() == "", h.last_error()
        h.close()
    assert seen == set(range(n))


def test_batches(hip_lib):
    import torch  # noqa: F401
    from test_gpu_mixed_batch import Seq, step
    from rgbd_util import RSeq, batch_step

    def solo_records(prm, sensor, frames):
        h = hip_lib.LvtSystem.create(prm, sensor)
        assert h.enable_pose_info(True) == 0
        out = []
        for f in frames:
            h.track(*f)
            out.append(h.pose_info())
        h.close()
        return out

    def check(batch, s, rec_solo, what):
        rec = batch.pose_info(s)
        assert rec.to_bytes() == rec_solo.to_bytes(), (what, rec.status, rec_solo.status, rec.frame, rec_solo.frame)
        return rec

    # a uniform batch of 3: sequences 0 and 1 the same drive, sequence 2 two frames ahead
    world, prm, _ = make_case("kitti", 0, 0.5)
    n = 6
    seqs = [Seq(world, prm, n), Seq(world, prm, n), Seq(world, prm, n, first=2)]
    solo = [solo_records(prm, 1, seqs[0].frames), None, solo_records(prm, 1, seqs[2].frames)]
    solo[1] = solo[0]
    batch = hip_lib.LvtBatch(prm, 3)
    assert batch.enable_pose_info(True) == 0, batch.last_error()
    for i in range(n):
        batch.track_device_async([q.ptrs(i)[0] for q in seqs], [q.ptrs(i)[1] for q in seqs], seqs[0].H, seqs[0].W, seqs[0].pitch)
        batch.wait()
        st = [check(batch, s, solo[s][i], f"uniform step {i} sequence {s}").status for s in range(3)]
        assert st == ([0, 0, 0] if i == 0 else [1, 1, 1]), (i, st)
    assert solo[0][3].to_bytes() != solo[2][3].to_bytes()
    with pytest.raises(IndexError):
        batch.pose_info(3)
    assert batch.last_error() == "", batch.last_error()
    batch.close()

    # a mixed batch of two calibrations, sequence 1 sitting step 3 out
    seqs = []
    for seed, size in ((70, (621, 187)), (72, (613, 185))):
        w, p, _ = make_case("kitti", seed, 1.0, None, size=size)
        seqs.append(Seq(w, p, n))
    solo = [solo_records(q.prm, 1, q.frames) for q in seqs]
    batch = hip_lib.LvtBatch.create_mixed([q.prm for q in seqs])
    assert batch.enable_pose_info(True) == 0, batch.last_error()
    nxt = [0, 0]
    for k in range(n):
        which = [nxt[0], None if k == 3 else nxt[1]]
        assert step(batch, seqs, which) == 0, batch.last_error()
        batch.wait()
        check(batch, 0, solo[0][which[0]], f"mixed step {k} sequence 0")
        if which[1] is None:
            assert batch.pose_info(1).status == 0
        else:
            assert check(batch, 1, solo[1][which[1]], f"mixed step {k} sequence 1").status == (1 if which[1] else 0)
        nxt = [nxt[0] + 1, nxt[1] + (0 if which[1] is None else 1)]
    assert batch.last_error() == "", batch.last_error()
    batch.close()

    # an RGB-D batch of 2
    seqs = [RSeq(86, {}, (320, 240), n), RSeq(86, {}, (320, 240), n, first=3)]
    solo = [solo_records(q.prm, 2, list(zip(q.gray, q.f32))) for q in seqs]
    batch = hip_lib.LvtBatch(seqs[0].prm, 2, sensor_type=2)
    assert batch.enable_pose_info(True) == 0, batch.last_error()
    for i in range(n):
        assert batch_step(batch, seqs, [i, i], hip_lib.DEPTH_F32, hip_lib) == 0, batch.last_error()
        batch.wait()
        for s in range(2):
            assert check(batch, s, solo[s][i], f"rgbd step {i} sequence {s}").status == (1 if i else 0)
    assert batch.last_error() == "", batch.last_error()
    batch.close()


def test_lost_and_reset(hip_lib):
    world, prm, _ = make_case("kitti", 0, 0.5)
    frames = [world.render_stereo(i) for i in range(8)]
    blank = np.full((world.H, world.W), 110, np.uint8)
    h = hip_lib.LvtSystem.create(prm, 1)
    assert h.enable_pose_info(True) == 0
    for i in range(4):
        h.track(*frames[i])
        assert h.pose_info().status == (1 if i else 0)
    h.track(blank, blank)
    assert h.get_state() == 3 and h.pose_info().status == 0
    h.track(*frames[5])                      # LOST is sticky
    assert h.get_state() == 3 and h.pose_info().status == 0
    h.reset()
    assert h.pose_info().status == 0 and h.pose_info().to_bytes() == bytes(hip_lib.POSE_INFO_SIZE)
    h.track(*frames[5])                      # the first tracked frame initialises the map: no pose of its own
    assert h.get_state() == 2 and h.pose_info().status == 0
    h.track(*frames[6])
    rec = h.pose_info()
    assert rec.status == 1 and rec.frame == h.counts()["frame"]
    h.close()


def test_launch_count(hip_lib):
    world, prm, _ = make_case("kitti", 0, 0.5)
    frames = [world.render_stereo(i) for i in range(4)]

    def rows_of(h):
        return [(name, calls) for name, _ms, calls in h.profile_read()]

    def run(h):
        h.profile_enable(True)
        for f in frames:
            h.track(*f)
        return rows_of(h)

    plain = hip_lib.LvtSystem.create(prm, 1)
    never = run(plain)
    assert never and not [n for n, _ in never if "k_pose_info" in n], never
    assert dict(never)["k_score"] == 4
    plain.close()
    h = hip_lib.LvtSystem.create(prm, 1)
    assert h.enable_pose_info(True) == 0
    on = run(h)
    assert dict(on)["k_pose_info"] == 4, on
    assert [(n, k) for n, k in on if n != "k_pose_info"] == never, (on, never)      # exactly one launch more per frame
    h.reset()
    assert h.enable_pose_info(False) == 0
    off = run(h)
    assert dict(off).get("k_pose_info", 0) == 0 and [(n, k) for n, k in off if n != "k_pose_info"] == never, (off, never)
    assert h.pose_info().status == 0
    h.close()


def test_snapshots(hip_lib):
    world, prm, _ = make_case("kitti", 0, 0.5)
    frames = [world.render_stereo(i) for i in range(8)]
    A = hip_lib.LvtSystem.create(prm, 1)
    assert A.enable_pose_info(True) == 0
    recs = []
    for i in range(3):
        A.track(*frames[i]); recs.append(A.pose_info())
    snap = A.snapshot()
    for i in range(3, 7):
        A.track(*frames[i]); recs.append(A.pose_info())
    assert recs[4].status == 1
    assert A.restore(snap) == 0, A.last_error()          # two (and more) frames later: back to the state after frame 2
    assert A.pose_info().status == 0 and A.pose_info().to_bytes() == bytes(hip_lib.POSE_INFO_SIZE)
    for i in range(3, 6):                                  # the continuation's records are the source's
        A.track(*frames[i])
        assert A.pose_info().to_bytes() == recs[i].to_bytes(), i
    # a fresh handle is not enabled by a snapshot from an enabled one ...
    B = hip_lib.LvtSystem.create(prm, 1)
    assert B.restore(snap) == 0, B.last_error()
    B.track(*frames[3])
    L = hip_lib.load_library()
    out = hip_lib.PoseInfo()
    assert L.lvt_amd_get_pose_info(ctypes.c_void_p(B._h), 0, ctypes.byref(out)) == 0 and out.to_bytes() == bytes(hip_lib.POSE_INFO_SIZE)
    B.close()
    # ... and its bytes are those of a never-enabled handle's snapshot of the same state
    C = hip_lib.LvtSystem.create(prm, 1)
    for i in range(3):
        C.track(*frames[i])
    plain = C.snapshot()
    assert plain.to_bytes() == snap.to_bytes()
    for x in (A, C, snap, plain):
        x.close()


def test_refusals(hip_lib, tmp_path):
    world, prm, _ = make_case("kitti", 0, 0.5)
    frames = [world.render_stereo(i) for i in range(3)]
    L = hip_lib.load_library()
    vp = ctypes.c_void_p
    out = hip_lib.PoseInfo()
    h = hip_lib.LvtSystem.create(prm, 1)
    # never enabled: 0 and a zeroed record
    h.track(*frames[0])
    ctypes.memset(ctypes.byref(out), 0xFF, hip_lib.POSE_INFO_SIZE)
    assert L.lvt_amd_get_pose_info(vp(h._h), 0, ctypes.byref(out)) == 0 and out.to_bytes() == bytes(hip_lib.POSE_INFO_SIZE)
    # seq out of range, no handle
    assert L.lvt_amd_get_pose_info(vp(h._h), 1, ctypes.byref(out)) == -1 and L.lvt_amd_get_pose_info(vp(h._h), -1, ctypes.byref(out)) == -1
    assert L.lvt_amd_get_pose_info(None, 0, ctypes.byref(out)) == -1 and L.lvt_amd_enable_pose_info(None, 1) == -1
    # frames in flight
    assert h.track_async(*frames[1]) == 0
    assert h.enable_pose_info(True) == -1 and "frames in flight" in h.last_error(), h.last_error()
    h.wait()
    assert h.enable_pose_info(True) == 0
    h.track(*frames[2])
    assert h.pose_info().status == 1
    h.close()
    # a pooled seat, automatic seats
    P = hip_lib.LvtSystem.create(prm, 1, pooled=True)
    assert P.enable_pose_info(True) == -1 and "pooled" in P.last_error(), P.last_error()
    assert L.lvt_amd_get_pose_info(vp(P._h), 0, ctypes.byref(out)) == 0 and out.status == 0
    P.track(*frames[0])
    assert P.get_state() == 2
    P.close()
    cfg = os.path.join(str(tmp_path), "cfg.yaml")
    prm.write_yaml(cfg)
    a1, a2 = hip_lib.LvtSystem.create_from_file(cfg, 1), hip_lib.LvtSystem.create_from_file(cfg, 1)
    assert a1.ordering() == a2.ordering() == "pooled"
    for a in (a1, a2):
        assert a.enable_pose_info(True) == -1 and "pooled" in a.last_error(), a.last_error()
    a1.close(); a2.close()
    # a lone lvt_create handle stays on its own chain and may enable it (a successful call is a use)
    lone = hip_lib.LvtSystem.create_from_file(cfg, 1)
    assert lone.enable_pose_info(True) == 0, lone.last_error()
    other = hip_lib.LvtSystem.create_from_file(cfg, 1)
    assert lone.ordering() != "pooled"
    lone.track(*frames[0]); lone.track(*frames[1])
    assert lone.pose_info().status == 1
    other.close(); lone.close()


def test_odometry_update_cov(hip_lib):
    """lvt_amd_odometry_update_cov = lvt_track + the frame's record + push_pose_cov: zeros for the first frame (no record), afterwards what a detached
    accumulator makes of the same pose and the handle's own record (the pose re-derived from the tracker's quaternion: a few ulp, hence 1e-9 relative)"""
    world, prm, _ = make_case("kitti", 0, 0.5)
    h = hip_lib.LvtSystem.create(prm, 1)
    assert h.enable_pose_info(True) == 0
    od, detached = hip_lib.Odometry(h), hip_lib.Odometry()
    for i in range(4):
        out = od.update_cov(*world.render_stereo(i), 0.1 * i)
        rec = h.pose_info()
        q, p = h.pose()
        want = detached.push_pose_cov(U.quat_to_R(q), p, 2, 0.1 * i, rec.cov if rec.status == 1 else None)
        assert out is not None and want is not None and rec.status == (1 if i else 0)
        assert np.abs(out[0] - want[0]).max() <= 1e-12 and np.abs(out[1] - want[1]).max() <= 1e-9
        assert np.abs(out[2] - want[2]).max() <= 1e-9 * max(np.abs(want[2]).max(), 1e-300), i
        assert out[2].any() == bool(i) and np.array_equal(out[2], out[2].T)
    plain = hip_lib.LvtSystem.create(prm, 1)          # never enabled: the covariance stays zero, pose and twist are update()'s
    od2 = hip_lib.Odometry(plain)
    for i in range(2):
        out = od2.update_cov(*world.render_stereo(i), 0.1 * i)
        assert out is not None and not out[2].any()
    for x in (od, od2, detached, h, plain):
        x.close()
