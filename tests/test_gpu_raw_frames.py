"""RAW stereo frames: a pair of rectifiers attached to a tracker (lvt_amd_set_rectifiers / lvt_amd_batch_set_rectifiers), rectification as the first
launch of the feature stage (k_rectify_frames).  Every expected value comes from the ORACLE chain the EuRoC command line test uses -- its own maps
(O.init_undistort_rectify_map), its own bilinear remap of every raw image (O.remap_bilinear), its tracker on those -- never from this library's
Rectifier.rectify.

The inputs are the smallest shapes at which the kernel can still go wrong:
  A   kitti world 71 at 621 x 187 (width = 1 mod 4; plane pitch 640: the last word of a row is part image, part padding), ONE pincushion rectifier for
      both eyes (K = P = the world's intrinsics, R = I): 11.6 % of the map samples outside the source -- the border and the partial 2 x 2 branches run
  B   the synthetic EuRoC world at 752 x 480 with the reference's cam0 / cam1 calibrations (a different map per eye)
  C   kitti world 32 at 620 x 188, a stronger pincushion (20.6 % of the map outside the source)
  C2  kitti world 32 at 613 x 185 with A's pincushion
The oracle chain of a case is computed once and shared by the tests that need it."""
import os
import tempfile

import numpy as np
import pytest

from parity_util import make_case, diff_frame, pose_errors, POSE_TOL

pytestmark = pytest.mark.gpu

PINCUSHION = [0.12, 0.02, 2e-4, -1e-4, 0.0]
PINCUSHION_C = [0.3, 0.0, 1e-3, -1e-3, 0.0]
EYE3 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
CAM1 = dict(K=[457.587, 0.0, 379.999, 0.0, 456.134, 255.238, 0.0, 0.0, 1.0], D=[-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0],
            R=[0.9999633526194376, -0.003625811871560086, 0.007755443660172947, 0.003680398547259526, 0.9999684752771629, -0.007035845251224894,
               -0.007729688520722713, 0.007064130529506649, 0.999945173484644])


class Case:
    """raw frames of a world, the two calibrations, the oracle's maps and rectified frames, and the oracle chain's record of every frame"""

    def __init__(self, world, prm, cals, n):
        from oracle import pyoracle as O
        self.world, self.prm, self.cals, self.n = world, prm, cals, n
        self.W, self.H = world.W, world.H
        self.pitch = ((self.W + 63) // 64) * 64
        self.raw = [tuple(np.ascontiguousarray(x) for x in world.render_stereo(i)) for i in range(n)]
        self.maps = [O.init_undistort_rectify_map(c["K"], c["D"], c["R"], c["P"], self.W, self.H) for c in cals]
        self.rect = [(O.remap_bilinear(a, *self.maps[0]), O.remap_bilinear(b, *self.maps[1])) for a, b in self.raw]
        self._chains = {}

    def oracle(self):
        from oracle import pyoracle as O
        return O.Oracle(self.prm, 1)

    def chain(self, first=0, n=8, rectified=True):
        """[(R, t, state, counts)] of the oracle over frames first .. first + n - 1 (rectified by the oracle, or as they are)"""
        key = (first, n, rectified)
        if key not in self._chains:
            orc, out = self.oracle(), []
            for i in range(first, first + n):
                R, t = orc.track(*(self.rect[i] if rectified else self.raw[i]))
                out.append((np.array(R), np.array(t), orc.status, orc.counts()))
            self._chains[key] = out
        return self._chains[key]

    def rectifiers(self, hip_lib):
        """(left, right) -- ONE object for both eyes when the calibrations are the same one"""
        rl = hip_lib.Rectifier(self.cals[0]["K"], self.cals[0]["D"], self.cals[0]["R"], self.cals[0]["P"], self.W, self.H)
        rr = rl if self.cals[1] is self.cals[0] else hip_lib.Rectifier(self.cals[1]["K"], self.cals[1]["D"], self.cals[1]["R"], self.cals[1]["P"], self.W, self.H)
        return rl, rr


_CASES = {}


def _world_cal(world, D):
    K = [world.fx, 0.0, world.cx, 0.0, world.fy, world.cy, 0.0, 0.0, 1.0]
    return dict(K=K, D=list(D), R=EYE3, P=K)


def get_case(name):
    if name in _CASES:
        return _CASES[name]
    import lvt_amd
    if name == "B":
        from lvt_amd.synth import make_world
        from test_oracle_primitives import EUROC_L
        world = make_world("euroc", seed=1)
        assert (world.W, world.H) == (752, 480)
        with tempfile.TemporaryDirectory() as d:   # the parameters as test_gpu_cli.py derives them: YAML floats, the calibration narrowed to float
            lvt_amd.euroc_params().write_yaml(os.path.join(d, "config.yaml"))
            prm = lvt_amd.LvtParameters.from_file(os.path.join(d, "config.yaml"))
        prm.fx = prm.fy = float(np.float32(435.2046959714599))
        prm.cx, prm.cy, prm.baseline = float(np.float32(367.4517211914062)), float(np.float32(252.2008514404297)), float(np.float32(0.110077842))
        prm.img_width, prm.img_height = 752, 480
        c = Case(world, prm, [EUROC_L, dict(CAM1, P=EUROC_L["P"])], 8)
    else:
        seed, size, D, n = {"A": (71, (621, 187), PINCUSHION, 9), "C": (32, (620, 188), PINCUSHION_C, 8), "C2": (32, (613, 185), PINCUSHION, 8)}[name]
        world, prm, _ = make_case("kitti", seed, size=size)
        cal = _world_cal(world, D)
        c = Case(world, prm, [cal, cal], n)
    _CASES[name] = c
    return c


def attached(hip_lib, c):
    hip = hip_lib.LvtSystem.create(c.prm, 1)
    rl, rr = c.rectifiers(hip_lib)
    assert hip.set_rectifiers(rl, rr) == 0, hip.last_error()
    return hip


def device_planes(frames, W, H, pitch, pad=255):
    """(n, 2, H, pitch) uint8 tensor in HBM; the padding columns hold `pad` (a raw plane's padding must never be sampled)"""
    import torch
    t = torch.full((len(frames), 2, H, pitch), pad, dtype=torch.uint8, device="cuda")
    for i, (a, b) in enumerate(frames):
        t[i, 0, :, :W] = torch.from_numpy(a).cuda(); t[i, 1, :, :W] = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    return t


def pinned(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy()


def close_to(R, t, ref, what):
    e_t, e_R = pose_errors(np.asarray(R), np.asarray(t), ref[0], ref[1])
    print(f"{what}: e_t {e_t:.2e} e_R {e_R:.2e}")
    assert e_t <= POSE_TOL and e_R <= POSE_TOL, f"{what}: e_t {e_t:.2e} e_R {e_R:.2e}"


def counts_equal(ch, co, what):
    bad = {k: (ch.get(k), v) for k, v in co.items() if ch.get(k) != v}
    assert not bad, f"{what}: counters (hip, oracle) {bad}"


# ---- 1. the rectified plane ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lvt_track", "track_device"])
@pytest.mark.parametrize("name,raw_pitch", [("A", 624), ("B", 752)])
def test_rectified_plane_equals_the_oracles_remap(hip_lib, oracle_lib, name, raw_pitch, route):
    """after one raw frame plane(eye, 2)[:, :W] is O.remap_bilinear(raw, the oracle's maps), byte for byte, and the padding columns are zero: through
    lvt_track (pageable buffers) and through lvt_amd_track_device with a raw pitch that is not the handle's"""
    c = get_case(name)
    hip = attached(hip_lib, c)
    if route == "lvt_track":
        hip.track(*c.raw[0])
    else:
        assert raw_pitch != c.pitch
        dev = device_planes(c.raw[:1], c.W, c.H, raw_pitch)
        hip.track_device(dev[0, 0].data_ptr(), dev[0, 1].data_ptr(), c.H, c.W, raw_pitch)
    assert hip.last_error() == "", hip.last_error()
    for eye in (0, 1):
        p = hip.plane(eye, 2)
        assert p.shape == (c.H, c.pitch) and p.dtype == np.uint8
        want = c.rect[0][eye]
        bad = np.argwhere(p[:, :c.W] != want)
        assert len(bad) == 0, f"eye {eye}: {len(bad)} pixels differ, first at {tuple(bad[0])}: hip {p[tuple(bad[0])]} oracle {want[tuple(bad[0])]}"
        assert not p[:, c.W:].any(), f"eye {eye}: the padding columns are not zero"
    outside = [float(np.mean((m1 < 0) | (m1 > c.W - 1) | (m2 < 0) | (m2 > c.H - 1))) for m1, m2 in c.maps]
    print("map entries outside the source:", outside)
    if name == "A":
        assert outside[0] > 0.05   # (a condition on the input: the border branches run)


def test_plane_2_of_a_plain_handle_is_empty(hip_lib, oracle_lib):
    c = get_case("A")
    hip = hip_lib.LvtSystem.create(c.prm, 1)
    hip.track(*c.rect[0])
    assert hip.plane(0, 2).size == 0 and hip.plane(0, 0).shape == (c.H, c.pitch)


# ---- 2. sequence parity, synchronous ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_raw_sequence_through_lvt_track_equals_the_oracle(hip_lib, oracle_lib, name):
    """8 raw frames through lvt_track: the complete frame diff against the oracle chain is empty on every frame, poses within POSE_TOL"""
    c = get_case(name)
    ref = c.chain(0, 8)
    assert [r[2] for r in ref] == [2] * 8, "the oracle is not TRACKING on all 8 frames: an early LOST would hide a difference"
    print("oracle features / matches:", [(r[3]["n_left"], r[3]["n_matches"]) for r in ref])
    hip, orc = attached(hip_lib, c), c.oracle()
    for i in range(8):
        Ro, to = orc.track(*c.rect[i])
        R, t = hip.track(*c.raw[i])
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"{name} frame {i}")


# ---- 3. sequence parity, asynchronous --------------------------------------------------------------------------------------------------
def _run_async(hip, submit, n, depth):
    got, inflight = [], 0
    for i in range(n):
        submit(i)
        inflight += 1
        if inflight >= depth:
            got.append(hip.wait_status()); inflight -= 1
    while inflight:
        got.append(hip.wait_status()); inflight -= 1
    return got


def _async_checks(c, hip, got):
    """state and pose of every collected frame against the oracle chain (the counters of a frame in flight cannot be read without draining the pipeline:
    they are compared, with the map and the staged set, through diff_frame behind the last frame -- as test_gpu_parity.py holds its asynchronous runs)"""
    ref = c.chain(0, 8)
    assert [r[2] for r in ref] == [2] * 8
    for i, (R, t, st) in enumerate(got):
        assert st == ref[i][2], f"frame {i}: state {st} oracle {ref[i][2]}"
        close_to(R, t, ref[i], f"frame {i}")
    orc = c.oracle()
    for i in range(8):
        orc.track(*c.rect[i])
    msgs = diff_frame(hip, orc)
    assert not msgs, msgs[:6]
    counts_equal(hip.counts(), ref[7][3], "last frame")


@pytest.mark.parametrize("memory", ["pageable", "page_locked"])
def test_raw_frames_through_track_async(hip_lib, oracle_lib, memory):
    """lvt_amd_track_async on raw host frames, four in flight: the staged planes (and the pull fused into the previous frame's corner-cell launch) carry
    raw bytes, the frame's feature stage rectifies them"""
    c = get_case("A")
    hip = attached(hip_lib, c)
    bufs = [(pinned(a), pinned(b)) if memory == "page_locked" else (a, b) for a, b in c.raw[:8]]

    def submit(i):
        assert hip.track_async(bufs[i][0], bufs[i][1]) == 0, hip.last_error()
    got = _run_async(hip, submit, 8, 4)
    _async_checks(c, hip, got)
    hs = hip.host_stats()
    assert hs["async_host_frames"] == 8 and (hs["planes_in_place"] if memory == "page_locked" else hs["planes_staged"]) == 16, hs


def test_raw_frames_through_track_device_async(hip_lib, oracle_lib):
    """raw planes in HBM with a pitch of their own (624: not the handle's 640), three frames in flight, read in place"""
    c = get_case("A")
    hip = attached(hip_lib, c)
    dev = device_planes(c.raw[:8], c.W, c.H, 624)
    got = _run_async(hip, lambda i: hip.track_device_async(dev[i, 0].data_ptr(), dev[i, 1].data_ptr(), c.H, c.W, 624), 8, 3)
    assert hip.last_error() == "", hip.last_error()
    _async_checks(c, hip, got)


# ---- 4. batches ------------------------------------------------------------------------------------------------------------------------
def test_uniform_batch_sharing_one_rectifier_pair(hip_lib, oracle_lib):
    """two sequences of case A in a uniform batch, both on ONE rectifier pair, one frame apart: state, pose and counters of every step"""
    c = get_case("A")
    batch = hip_lib.LvtBatch(c.prm, 2)
    rl, rr = c.rectifiers(hip_lib)
    assert batch.set_rectifiers(0, rl, rr) == 0 and batch.set_rectifiers(1, rl, rr) == 0, batch.last_error()
    dev = device_planes(c.raw, c.W, c.H, 624)
    refs = [c.chain(0, 8), c.chain(1, 8)]
    for k in range(8):
        batch.track_device_async([dev[k, 0].data_ptr(), dev[k + 1, 0].data_ptr()], [dev[k, 1].data_ptr(), dev[k + 1, 1].data_ptr()], c.H, c.W, 624)
        R, t, st = batch.wait()
        assert batch.last_error() == "", batch.last_error()
        for s in range(2):
            assert st[s] == refs[s][k][2], f"sequence {s} step {k}: state {st[s]} oracle {refs[s][k][2]}"
            close_to(R[s], t[s], refs[s][k], f"sequence {s} step {k}")
            counts_equal(batch.counts(s), refs[s][k][3], f"sequence {s} step {k}")


@pytest.mark.parametrize("depth", [3, 1], ids=["three_in_flight", "counters_of_every_step"])
def test_mixed_batch_raw_plain_and_absent(hip_lib, oracle_lib, depth):
    """a mixed batch of three over 8 steps: sequence 0 = case C, raw; sequence 1 = case A's world WITHOUT rectifiers, fed its frames as they are;
    sequence 2 = case C2, raw, present for steps 0 - 4 and absent afterwards (it repeats its last record).  Every sequence against its own oracle
    chain: state and pose of every step with three steps in flight; one step at a time, the counters of every step as well (reading them drains)"""
    cs = [get_case("C"), get_case("A"), get_case("C2")]
    batch = hip_lib.LvtBatch([c.prm for c in cs])
    keep = []
    for s in (0, 2):
        keep.append(cs[s].rectifiers(hip_lib))
        assert batch.set_rectifiers(s, *keep[-1]) == 0, batch.last_error()
    pitches = [620, cs[1].pitch, 613]   # raw planes: tightly packed, an odd pitch; the rectified sequence keeps the pitch % 16 rule
    devs = [device_planes(c.raw[:8], c.W, c.H, p, pad=(0 if s == 1 else 255)) for s, (c, p) in enumerate(zip(cs, pitches))]
    refs = [cs[0].chain(0, 8), cs[1].chain(0, 8, rectified=False), cs[2].chain(0, 5)]
    got, cnt, inflight = [], [], 0

    def collect():
        got.append(batch.wait())
        if depth == 1:
            cnt.append([batch.counts(s) for s in range(3)])
    for k in range(8):
        here = [True, True, k < 5]
        lp = [devs[s][k, 0].data_ptr() if here[s] else None for s in range(3)]
        rp = [devs[s][k, 1].data_ptr() if here[s] else None for s in range(3)]
        assert batch.track_device_async_mixed(lp, rp, [c.H for c in cs], [c.W for c in cs], pitches) == 0, batch.last_error()
        inflight += 1
        if inflight >= depth:
            collect(); inflight -= 1
    while inflight:
        collect(); inflight -= 1
    assert batch.last_error() == "", batch.last_error()
    for s in range(3):
        for k in range(8):
            ref = refs[s][min(k, len(refs[s]) - 1)]   # (an absent sequence: its last frame's record)
            R, t, st = got[k]
            assert st[s] == ref[2], f"sequence {s} step {k}: state {st[s]} oracle {ref[2]}"
            close_to(R[s], t[s], ref, f"sequence {s} step {k}")
            if k >= 5 and s == 2:
                assert np.array_equal(R[s], got[4][0][s]) and np.array_equal(t[s], got[4][1][s]), f"step {k}: the absent sequence's record changed"
            if depth == 1:
                counts_equal(cnt[k][s], ref[3], f"sequence {s} step {k}")
        counts_equal(batch.counts(s), refs[s][-1][3], f"sequence {s} after the last step")


# ---- 5. launch accounting --------------------------------------------------------------------------------------------------------------
def _profile_of(h):
    return [(name, calls) for name, _ms, calls in h.profile_read()]


def test_launch_accounting(hip_lib, oracle_lib):
    """a plain handle launches what it always did (no k_rectify_frames slot; slot names and call counts those of a second plain handle); an attached
    handle: one k_rectify_frames call per frame; a batch step: ONE call whatever the number of raw sequences, none when no raw sequence has a frame"""
    c = get_case("A")
    plain = []
    for _ in range(2):
        hip = hip_lib.LvtSystem.create(c.prm, 1)
        hip.profile_enable(True)
        for i in range(4):
            hip.track(*c.rect[i])
        plain.append(_profile_of(hip))
        hip.close()
    assert plain[0] == plain[1] and plain[0], plain
    assert not [n for n, _ in plain[0] if "k_rectify_frames" in n], plain[0]
    assert dict(plain[0])["k_score"] == 4

    hip = attached(hip_lib, c)
    hip.profile_enable(True)
    for i in range(4):
        hip.track(*c.raw[i])
    prof = _profile_of(hip)
    assert dict(prof)["k_rectify_frames"] == 4, prof
    assert [(n, k) for n, k in prof if n != "k_rectify_frames"] == plain[0], (prof, plain[0])   # ... and nothing else changed

    batch = hip_lib.LvtBatch(c.prm, 3)
    rl, rr = c.rectifiers(hip_lib)
    for s in (0, 2):
        assert batch.set_rectifiers(s, rl, rr) == 0, batch.last_error()
    raw = device_planes(c.raw[:2], c.W, c.H, c.pitch)
    rect = device_planes(c.rect[:2], c.W, c.H, c.pitch, pad=0)
    batch.profile_enable(True)
    dims = ([c.H] * 3, [c.W] * 3, [c.pitch] * 3)
    assert batch.track_device_async_mixed([raw[0, 0].data_ptr(), rect[0, 0].data_ptr(), raw[0, 0].data_ptr()],
                                          [raw[0, 1].data_ptr(), rect[0, 1].data_ptr(), raw[0, 1].data_ptr()], *dims) == 0, batch.last_error()
    batch.wait()
    assert dict(_profile_of(batch))["k_rectify_frames"] == 1, _profile_of(batch)
    assert batch.track_device_async_mixed([None, rect[1, 0].data_ptr(), None], [None, rect[1, 1].data_ptr(), None], *dims) == 0, batch.last_error()
    batch.wait()
    prof = dict(_profile_of(batch))
    assert prof["k_rectify_frames"] == 1 and prof["k_score"] == 2, prof
    assert batch.last_error() == "", batch.last_error()


def test_a_batch_with_more_raw_sequences_than_one_table_holds(hip_lib, oracle_lib):
    """33 raw stereo sequences on ONE rectifier pair = 66 images: the step takes a second k_rectify_frames launch (sequence 32's two images).  Sequence s
    starts at frame s % 3 of case A; three steps; sequences 0, 1, 31 and 32 against their oracle chains (state, pose, all counters), every sequence TRACKING"""
    c = get_case("A")
    B, steps = 33, 3
    batch = hip_lib.LvtBatch(c.prm, B)
    rl, rr = c.rectifiers(hip_lib)
    for s in range(B):
        assert batch.set_rectifiers(s, rl, rr) == 0, batch.last_error()
    dev = device_planes(c.raw[:steps + 2], c.W, c.H, 624)
    refs = [c.chain(o, steps) for o in range(3)]
    assert all(r[2] == 2 for ref in refs for r in ref), "the oracle is not TRACKING on every frame: an early LOST would hide a difference"
    batch.profile_enable(True)
    for k in range(steps):
        fr = [k + s % 3 for s in range(B)]
        batch.track_device_async([dev[i, 0].data_ptr() for i in fr], [dev[i, 1].data_ptr() for i in fr], c.H, c.W, 624)
        R, t, st = batch.wait()
        assert batch.last_error() == "", batch.last_error()
        assert list(st) == [2] * B, (k, list(st))
        for s in (0, 1, 31, 32):
            ref = refs[s % 3][k]
            assert st[s] == ref[2]
            close_to(R[s], t[s], ref, f"sequence {s} step {k}")
            counts_equal(batch.counts(s), ref[3], f"sequence {s} step {k}")
    assert dict(_profile_of(batch))["k_rectify_frames"] == steps   # (the slot times a step's first launch)


# ---- 6. refusals and detach ------------------------------------------------------------------------------------------------------------
def test_refused_attachments(hip_lib, oracle_lib, tmp_path):
    """every refusal returns -1 with a reason and leaves the handle as it was"""
    c, c2 = get_case("A"), get_case("C2")
    rl, rr = c.rectifiers(hip_lib)
    other_size = c2.rectifiers(hip_lib)[0]

    def refused(h, rc):
        assert rc == -1 and h.last_error() != "", (rc, h.last_error())

    hip = hip_lib.LvtSystem.create(c.prm, 1)
    refused(hip, hip.set_rectifiers(other_size, other_size))             # width / height not the sequence's
    refused(hip, hip.set_rectifiers(rl, None)); refused(hip, hip.set_rectifiers(None, rr))   # one NULL
    hip.track(*c.rect[0])                                                 # still a plain, usable handle
    assert hip.get_state() == 2 and hip.plane(0, 2).size == 0
    dev = device_planes(c.rect[1:2], c.W, c.H, c.pitch, pad=0)
    hip.track_device_async(dev[0, 0].data_ptr(), dev[0, 1].data_ptr(), c.H, c.W, c.pitch)
    refused(hip, hip.set_rectifiers(rl, rr))                             # a frame in flight
    assert "in flight" in hip.last_error()
    _, _, st = hip.wait_status()
    assert st == 2
    assert hip.set_rectifiers(rl, rr) == 0, hip.last_error()              # everything collected: accepted
    assert hip.set_rectifiers(None, None) == 0

    tw, tp, _ = make_case("tum", 4, 0.5)
    rgbd = hip_lib.LvtSystem.create(tp, 2)
    rt = hip_lib.Rectifier(_world_cal(tw, PINCUSHION)["K"], PINCUSHION, EYE3, _world_cal(tw, PINCUSHION)["K"], tw.W, tw.H)
    refused(rgbd, rgbd.set_rectifiers(rt, rt))                            # an RGB-D handle
    assert rgbd.get_state() == 1

    seat = hip_lib.LvtSystem.create(c.prm, 1, pooled=True)
    assert seat.ordering() == "pooled"
    refused(seat, seat.set_rectifiers(rl, rr))                           # a pooled seat
    seat.track(*c.rect[0])
    assert seat.get_state() == 2
    seat.close()

    c.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    autos = [hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1) for _ in range(2)]
    assert autos[0].ordering() == "pooled"
    refused(autos[0], autos[0].set_rectifiers(rl, rr))                   # an automatic seat
    assert autos[0].get_state() == 1
    for a in autos:
        a.close()

    batch = hip_lib.LvtBatch(c.prm, 2)
    for seq in (-1, 2):
        refused(batch, batch.set_rectifiers(seq, rl, rr))               # seq out of range
    refused(batch, hip_lib.load_library().lvt_amd_set_rectifiers(batch._h, rl._h, rr._h))   # the solo call on a batch
    refused(batch, batch.set_rectifiers(0, other_size, other_size))
    assert batch.set_rectifiers(1, rl, rr) == 0, batch.last_error()


def test_rectifier_of_another_device_is_refused(hip_lib, oracle_lib):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    c = get_case("A")
    with torch.cuda.device(1):
        rl, rr = c.rectifiers(hip_lib)
    hip = hip_lib.LvtSystem.create(c.prm, 1, device=0)
    assert hip.set_rectifiers(rl, rr) == -1 and "device" in hip.last_error()
    hip.track(*c.rect[0])
    assert hip.get_state() == 2


def test_external_corners_are_refused_on_an_attached_handle(hip_lib, oracle_lib):
    c = get_case("A")
    hip = attached(hip_lib, c)
    hip.track(*c.raw[0])
    before = (hip.counts(), hip.get_state(), hip.pose())
    corners = np.array([[100.0, 50.0], [200.0, 80.0]])
    hip.track_with_external_corners(c.raw[1][0], c.raw[1][1], corners, corners)
    assert "external_corners" in hip.last_error()
    after = (hip.counts(), hip.get_state(), hip.pose())
    assert before[0] == after[0] and before[1] == after[1] == 2, (before[0]["frame"], after[0]["frame"])
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1], after[2][1])
    R, t = hip.track(*c.raw[1])                                            # the handle goes on with the next raw frame
    close_to(R, t, c.chain(0, 8)[1], "the frame after the refusal")


def test_attach_then_detach_leaves_a_plain_handle(hip_lib, oracle_lib):
    """detached before the first frame: 4 frames equal the oracle on the frames AS GIVEN"""
    c = get_case("A")
    hip = attached(hip_lib, c)
    assert hip.set_rectifiers(None, None) == 0
    orc = c.oracle()
    for i in range(4):
        orc.track(*c.raw[i])
        hip.track(*c.raw[i])
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
    assert hip.plane(0, 2).size == 0


def test_an_attach_is_a_use_of_an_lvt_create_handle(hip_lib, oracle_lib, tmp_path):
    """lvt_create, set_rectifiers, a second lvt_create with the same parameters: the first handle keeps its own chain"""
    c = get_case("A")
    c.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    first = hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1)
    rl, rr = c.rectifiers(hip_lib)
    assert first.set_rectifiers(rl, rr) == 0, first.last_error()
    second = hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1)
    assert first.ordering() != "pooled" and hip_lib.load_library().lvt_amd_get_ordering(first._h) != 2
    first.track(*c.raw[0])
    want = c.rect[0][0]
    assert np.array_equal(first.plane(0, 2)[:, :c.W], want)
    second.close(); first.close()
