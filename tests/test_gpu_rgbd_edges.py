"""The RGB-D feature gather at its depth and lens edges: what only an RGB-D frame reaches -- the depth lookup and the near / far filter of k_gather,
its 16-bit conversion, undistort_point with the "left the hash grid -> drop" rule, the fp32 back-projection of k_triangulate -- on inputs
constructed for it (case_tables.py; test_case_tables.py holds them to their conditions with the oracle alone).  Every image is 640 x 480.

  planted depth, fp32   15 classes of depth (NaN, the infinities, negatives, both zeros, a denormal, both planes with their fp32 neighbours, 3.4e38)
                        written at the 804 corners of frame 0: the features are the 266 corners numpy float32 keeps by near <= d <= far, in list order,
                        and the map EQUALS the fp32 restatement of the back-projection.  Host call, device planes with a padded depth pitch, batch step
  planted depth, 16-bit two sets of raws whose pinned raw (2500 at 1/5000, 5000 at 0.001) falls on a plane by the rounding of ONE fp32 multiply and
                        beside it under any wider product; host call, device plane at an odd 2-byte address, and the fp32 conversion bit for bit
  barrel distortion     k1 < 0: on every frame features kept at x in [640, 650), corners dropped for leaving the hash grid, matches on the former
  retry pass            fewer than 200 corners: k_gather's in-kernel second detection pass on an RGB-D handle (eye 1 leaves early)
  no valid depth        an all-NaN first frame; an all-zero frame in mid-sequence, as fp32 and as 16-bit raw 0
  batch                 the planted sequence and the barrel sequence as one mixed lock-step batch

The comparison is parity_util.diff_frame against the oracle (integer stages bit-exact, XYZ_TOL) and POSE_TOL on the pose, on every frame.  The oracle
runs once per case; its state behind every frame is kept and shared by the routes."""
import numpy as np
import pytest

from case_tables import (RGBD_BARREL, RGBD_BARREL_FRAMES, RGBD_NODEPTH, RGBD_RETRY, RGBD_RETRY_FRAMES, rgbd_backproject, rgbd_nodepth_script, rgbd_outside,
                         rgbd_planted, rgbd_world)
from parity_util import POSE_TOL, diff_frame, pose_errors
from rgbd_util import SCALE, RSeq, batch_step, need, record, same_records

pytestmark = pytest.mark.gpu

TRACKING, LOST = 2, 3


class OracleFrame:
    """the oracle's state behind one frame, kept: diff_frame reads it like the live oracle"""

    def __init__(self, orc, R, t):
        self.R, self.t, self.status = R.copy(), t.copy(), orc.status
        self._counts, self._feat = orc.counts(), [orc.features(0), orc.features(1)]
        self._matches, self._rows, self._map, self._staged, self._pred = orc.matches(), orc.row_matches(), orc.map(), orc.staged(), orc.predicted_pose()

    def counts(self):
        return dict(self._counts)

    def features(self, eye=0):
        return self._feat[eye]

    def matches(self):
        return self._matches

    def row_matches(self):
        return self._rows

    def map(self):
        return self._map

    def staged(self):
        return self._staged

    def predicted_pose(self):
        return self._pred


_CASES = {}


def case(oracle_lib, key):
    """(prm, frames = [(gray, depth plane as handed in, its fp32 value)], depth scale of the 16-bit planes, [OracleFrame per frame]); made once"""
    if key not in _CASES:
        scale = SCALE
        if key[0] == "planted":
            c = rgbd_planted(key[1])
            prm, frames, scale = c["prm"], c["frames"], c["scale"]
        elif key[0] == "nodepth":
            prm, frames, _ = rgbd_nodepth_script(key[1])
        else:
            world, prm = rgbd_world({"barrel": RGBD_BARREL, "retry": RGBD_RETRY}[key[0]])
            frames = []
            for i in range({"barrel": RGBD_BARREL_FRAMES, "retry": RGBD_RETRY_FRAMES}[key[0]]):
                g, d = world.render_rgbd(i)
                d = np.ascontiguousarray(d, dtype=np.float32)
                frames.append((np.ascontiguousarray(g), d, d))
        orc = oracle_lib.Oracle(prm, 2)
        ref = []
        for g, _, f in frames:
            R, t = orc.track_rgbd(g, f)
            ref.append(OracleFrame(orc, R, t))
        _CASES[key] = (prm, frames, scale, ref)
    return _CASES[key]


def hold(hip, ref, R, t, what):
    """the stage diff and the pose of one frame; prints the figures first"""
    msgs = diff_frame(hip, ref)
    e_t, e_R = pose_errors(R, t, ref.R, ref.t)
    c = hip.counts()
    print(f"{what}: state {hip.get_state()} / {ref.status} n_left {c['n_left']} matches {c['n_matches']} map {c['map_size']} e_t {e_t:.2e} e_R {e_R:.2e}")
    assert not msgs, f"{what}: {msgs}"
    assert e_t <= POSE_TOL and e_R <= POSE_TOL, f"{what}: pose e_t {e_t:.2e} e_R {e_R:.2e}"
    assert hip.last_error() == "", hip.last_error()


def run_host(hip_lib, prm, frames, scale, ref, what, on_frame=None):
    """the synchronous host calls (lvt_amd_track_rgbd for an fp32 plane, lvt_amd_track_rgbd16 for a uint16 one), every frame held to the oracle"""
    hip = hip_lib.LvtSystem.create(prm, 2)
    out = []
    for i, (g, handed, _) in enumerate(frames):
        R, t = hip.track(g, handed, depth_scale=scale)
        hold(hip, ref[i], R, t, f"{what} frame {i}")
        if on_frame:
            on_frame(i, hip)
        out.append(record(hip, R, t))
    return out


def run_device(hip_lib, q, fmt, scale, ref, what, on_frame=None):
    """lvt_amd_track_rgbd_device on planes in HBM: fp32 with a depth pitch larger than the row (the padding holds 3.0, a valid depth), or 16-bit at an
    odd 2-byte address with a padded pitch"""
    hip = hip_lib.LvtSystem.create(q.prm, 2)
    out = []
    for i in range(q.n):
        if fmt == hip_lib.DEPTH_U16:
            assert q.u16_ptr(i) % 4 == 2 and q.u16_pitch() > 2 * q.W
            r = hip.track_rgbd_device(q.gray_ptr(i), q.u16_ptr(i), q.H, q.W, q.gpitch, q.u16_pitch(), fmt, scale)
        else:
            assert q.f32_pitch() > 4 * q.W
            r = hip.track_rgbd_device(q.gray_ptr(i), q.f32_ptr(i), q.H, q.W, q.gpitch, q.f32_pitch(), fmt)
        assert r is not None, hip.last_error()
        hold(hip, ref[i], r[0], r[1], f"{what} frame {i}")
        if on_frame:
            on_frame(i, hip)
        out.append(record(hip, *r))
    return out


def planted_checks(c, ref):
    """frame 0 of a planted case three ways: the oracle = the numpy restatement here, HIP = the numpy restatement in the returned hook, HIP = the oracle
    in hold().  The restatement: the corners numpy float32 keeps by near <= d <= far, in list order, with their compute_features descriptors; the map
    array_equal, not close, to the widened fp32 back-projection."""
    k = c["keep"]
    want_xy, want_desc, want_map = c["xy"][k], c["desc"][k], rgbd_backproject(c["prm"], c["xy"][k], c["val"][k])

    def equals_restatement(system, who):
        xy, _, desc = system.features(0)
        assert len(xy) == int(k.sum()), f"{who}: {len(xy)} features, numpy float32 keeps {int(k.sum())} of {len(k)}"
        assert np.array_equal(xy, want_xy) and np.array_equal(desc, want_desc), f"{who}: not the kept corners in list order"
        m = system.map()
        assert m[0].shape == want_map.shape and np.array_equal(m[0], want_map), f"{who}: the map is not the fp32 back-projection"
        assert np.array_equal(m[3], want_desc) and system.counts()["n_right"] == 0

    equals_restatement(ref[0], "oracle")
    return lambda i, hip: equals_restatement(hip, "hip") if i == 0 else None


def test_planted_depth_f32_host(hip_lib, oracle_lib):
    """NaN, +-inf, -1, -0.0, 0.0, 1e-45, near-, far+ and 3.4e38 are dropped, near, near+, 1.5, far- and far are kept: 266 of 804, through lvt_amd_track_rgbd;
    frames 1 - 3 track the world's own depth on that map"""
    c = rgbd_planted("f32")
    prm, frames, scale, ref = case(oracle_lib, ("planted", "f32"))
    assert int(c["keep"].sum()) == 266 and len(c["keep"]) == 804 and len(frames) == 4
    run_host(hip_lib, prm, frames, scale, ref, "host fp32", planted_checks(c, ref))
    assert all(r.status == TRACKING for r in ref)


def test_planted_depth_f32_device_padded_pitch(hip_lib, oracle_lib):
    """the same frames as device planes whose depth rows are 12 elements longer than the image: the planted pixel is found through the pitch"""
    need(hip_lib, "lvt_amd_track_rgbd_device")
    c = rgbd_planted("f32")
    prm, frames, scale, ref = case(oracle_lib, ("planted", "f32"))
    q = RSeq.from_frames(prm, [f[0] for f in frames], [f[2] for f in frames])
    run_device(hip_lib, q, hip_lib.DEPTH_F32, 1.0, ref, "device fp32", planted_checks(c, ref))


@pytest.mark.parametrize("name", ["A", "B"])
def test_planted_depth_u16(hip_lib, oracle_lib, name):
    """raw classes in a uint16 plane, expected through numpy raw.astype(float32) * float32(scale).  Set A (scale 1/5000): raw 2500 is exactly near in fp32
    and kept, below near in any wider product.  Set B (scale 0.001): raw 5000 is exactly far in fp32 and kept, above far in any wider product.  Through
    lvt_amd_track_rgbd16, through the device entry with the plane at an odd 2-byte address, and bit-identical to the fp32 conversion handed in"""
    need(hip_lib, "lvt_amd_track_rgbd16", "lvt_amd_track_rgbd_device")
    c = rgbd_planted(name)
    prm, frames, scale, ref = case(oracle_lib, ("planted", name))
    pinned = {"A": 2500, "B": 5000}[name]
    u0 = frames[0][1][c["xy"][:, 1].astype(int), c["xy"][:, 0].astype(int)]
    assert frames[0][1].dtype == np.uint16 and c["keep"][u0 == pinned].all() and (u0 == pinned).sum() > 50
    host16 = run_host(hip_lib, prm, frames, scale, ref, f"host u16 {name}", planted_checks(c, ref))
    q = RSeq.from_frames(prm, [f[0] for f in frames], [f[2] for f in frames], [f[1] for f in frames])
    dev16 = run_device(hip_lib, q, hip_lib.DEPTH_U16, scale, ref, f"device u16 {name}", planted_checks(c, ref))
    host32 = run_host(hip_lib, prm, [(g, f, f) for g, _, f in frames], None, ref, f"host fp32 of {name}", planted_checks(c, ref))
    same_records(host16, host32, "host u16 vs host fp32")
    same_records(dev16, host32, "device u16 vs host fp32")


def test_barrel_distortion(hip_lib, oracle_lib):
    """k1 = -0.283 (barrel): every key point moves outwards.  On each of 8 frames at least 5 features are kept outside [0, 640) x [0, 480), at least 5 corners
    are dropped for leaving the hash grid, and over the sequence map points are matched to features outside the image; the stage diff holds throughout"""
    prm, frames, scale, ref = case(oracle_lib, ("barrel",))
    assert prm.k1 < 0 and len(frames) == 8
    seen = []

    def conditions(i, hip):
        xy = hip.features(0)[0]
        out = rgbd_outside(xy)
        fi, _ = hip.matches()
        c = hip.counts()
        drops = len(oracle_lib.compute_features(frames[i][0], prm)[0]) - c["n_left"]      # (the depth plane is valid everywhere)
        seen.append((c["n_matches"], int(out.sum()), drops, int(out[fi].sum())))
        assert hip.get_state() == TRACKING and (i == 0 or c["n_matches"] > 600), (i, c)
        assert out.sum() >= 5 and drops >= 5, (i, seen[-1])

    run_host(hip_lib, prm, frames, scale, ref, "barrel", conditions)
    print("matches, kept outside the image, dropped by the grid rule, matches on a feature outside the image:", seen)
    assert sum(s[3] for s in seen) >= 1


def test_retry_pass_on_rgbd(hip_lib, oracle_lib):
    """agast_threshold 150 leaves 159 - 181 corners: the second detection pass runs inside k_gather for eye 0 while eye 1 of the RGB-D handle leaves early"""
    prm, frames, scale, ref = case(oracle_lib, ("retry",))

    def conditions(i, hip):
        c = hip.counts()
        assert c["retry_left"] == 1 and c["n_right"] == 0 and 0 < c["n_left"] < 200 and hip.get_state() == TRACKING, (i, c)

    run_host(hip_lib, prm, frames, scale, ref, "retry", conditions)
    assert len(frames) == 4 and all(r.status == TRACKING and r.counts()["retry_left"] == 1 for r in ref)


@pytest.mark.parametrize("name", sorted(RGBD_NODEPTH))
def test_frames_without_valid_depth(hip_lib, oracle_lib, name):
    """nan_first: an all-NaN first frame leaves no feature and an empty map, reports TRACKING and is LOST from the next frame on.  zero_mid / zero16_mid:
    an all-zero frame (fp32 / 16-bit raw 0) behind two good ones ends in the LOST latch.  Status sequence, counters and the stage diff on every frame"""
    prm, frames, scale, ref = case(oracle_lib, ("nodepth", name))
    kinds, status = RGBD_NODEPTH[name]
    assert [r.status for r in ref] == list(status)
    states = []

    def conditions(i, hip):
        states.append(hip.get_state())
        c = hip.counts()
        if kinds[i] != "world":
            assert c["n_left"] == 0 and c["n_matches"] == 0, (i, c)
        if name == "nan_first":
            assert c["map_size"] == 0, (i, c)

    run_host(hip_lib, prm, frames, scale, ref, name, conditions)
    assert states == list(status) and LOST in states


def test_mixed_batch_planted_and_barrel(hip_lib, oracle_lib):
    """k_gather's batch form: sequence 0 is the planted fp32 case (the planted plane in step 0, the world's depth afterwards), sequence 1 the barrel case;
    4 lock-step steps on device planes with padded depth pitches, each sequence held to its own oracle behind every step"""
    need(hip_lib, "lvt_amd_batch_track_rgbd_device_async")
    steps = 4
    refs, seqs = [], []
    for key in (("planted", "f32"), ("barrel",)):
        prm, frames, _, ref = case(oracle_lib, key)
        seqs.append(RSeq.from_frames(prm, [f[0] for f in frames[:steps]], [f[2] for f in frames[:steps]]))
        refs.append(ref)
    assert seqs[0].prm.far_plane_distance == 5.0 and seqs[0].prm.k1 == 0 and seqs[1].prm.k1 < 0 and seqs[0].f32_pitch() > 4 * seqs[0].W
    batch = hip_lib.LvtBatch.create_mixed([q.prm for q in seqs], sensor_type=2)
    for k in range(steps):
        assert batch_step(batch, seqs, [k, k], hip_lib.DEPTH_F32, hip_lib) == 0, batch.last_error()
        R, t, st = batch.wait()
        assert batch.last_error() == "", batch.last_error()
        for s in range(2):
            ref = refs[s][k]
            e_t, e_R = pose_errors(R[s], t[s], ref.R, ref.t)
            co, ch = ref.counts(), batch.counts(s)
            print(f"sequence {s} step {k}: state {st[s]} / {ref.status} n_left {ch['n_left']} matches {ch['n_matches']} map {ch['map_size']} e_t {e_t:.2e} e_R {e_R:.2e}")
            bad = {n: (ch.get(n), v) for n, v in co.items() if ch.get(n) != v}
            assert not bad, f"sequence {s} step {k}: counters (hip, oracle) {bad}"
            assert not ch["overflow"] and st[s] == ref.status == TRACKING, (s, k, st[s], ref.status)
            assert e_t <= POSE_TOL and e_R <= POSE_TOL, f"sequence {s} step {k}: pose e_t {e_t:.2e} e_R {e_R:.2e}"
        if k == 0:
            c0 = batch.counts(0)
            assert c0["n_left"] == 266 and c0["map_size"] == 266, c0
