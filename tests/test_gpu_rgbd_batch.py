"""RGB-D beyond the two host fp32 calls: frames already in HBM (lvt_amd_track_rgbd_device[_async]), 16-bit depth (lvt_amd_track_rgbd16[_async],
LVT_AMD_DEPTH_U16) and lock-step RGB-D batches, uniform and mixed (lvt_amd_batch_track_rgbd_device_async).

Inputs: worlds from make_case("tum", seed, 1.0, overrides, size); 16-bit depth u = clip(rint(d * 5000), 0, 65535) as uint16, scale
s = float32(1) / float32(5000); the oracle and every fp32 entry get u.astype(float32) * s -- the one rounded fp32 multiply the 16-bit path does where
it has key points, so 16-bit and fp32 runs must agree BIT FOR BIT, and everything is held to the CPU oracle frame by frame (POSE_TOL, equal states,
equal counters, the oracle TRACKING on every frame).  Two patches written into u (a hole of raw 0 = "no depth", a block of raw 30000 = 6 m, beyond
far_plane_distance 5.0) make the depth filter visibly act: n_left falls from ~810 to 637-671 (seed 80).

Every test first asserts that the symbols it needs exist, before any handle is used."""
import ctypes as C

import numpy as np
import pytest

from parity_util import make_case, pose_errors, diff_frame, POSE_TOL
from rgbd_util import SCALE, RSeq, batch_run, batch_step, check_against_own_oracles, need, record, run_host_f32, same_records

pytestmark = pytest.mark.gpu

FR1_DISTORTION = {"k1": 0.262383, "k2": -0.953104, "p1": -0.005358, "p2": 0.002628, "k3": 1.163314}
MIXED_CASES = [(84, FR1_DISTORTION, (640, 480)), (85, {"detection_cell_size": 300}, (640, 480)), (86, {}, (320, 240)), (87, {"tracking_radius": 45}, (800, 600))]


def test_device_equals_host_one_handle(hip_lib, oracle_lib):
    """fp32 planes in HBM through lvt_amd_track_rgbd_device == the same arrays through lvt_amd_track_rgbd, bit for bit, and both == the oracle"""
    need(hip_lib, "lvt_amd_track_rgbd_device", "lvt_amd_track_rgbd_device_async")
    q = RSeq(80, {}, (640, 480), 16)
    dev = hip_lib.LvtSystem.create(q.prm, 2)
    orc = oracle_lib.Oracle(q.prm, 2)
    got = []
    for i in range(q.n):
        tight = (i % 2 == 1)   # (a depth pitch larger than the row on the even frames, the tight one on the odd ones)
        res = dev.track_rgbd_device(q.gray_ptr(i), q.f32_ptr(i, tight), q.H, q.W, q.gpitch, q.f32_pitch(tight), hip_lib.DEPTH_F32)
        assert res is not None, dev.last_error()
        R, t = res
        Ro, to = orc.track_rgbd(q.gray[i], q.f32[i])
        msgs = diff_frame(dev, orc)
        e_t, e_R = pose_errors(R, t, Ro, to)
        print(f"frame {i}: e_t {e_t:.2e} e_R {e_R:.2e} state {orc.status}")
        assert not msgs, f"frame {i}: {msgs}"
        assert e_t <= POSE_TOL and e_R <= POSE_TOL, f"frame {i}: {e_t:.2e} {e_R:.2e}"
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        got.append(record(dev, R, t))
    assert dev.last_error() == "", dev.last_error()
    same_records(got, run_host_f32(hip_lib, q), "device fp32 vs host fp32")


def test_u16_equals_f32(hip_lib, oracle_lib):
    """16-bit depth through the synchronous host entry, the asynchronous host entry (three frames in flight) and the device entry (odd 2-byte address,
    padded pitch): each bit-identical to the fp32 host entry fed u * s; that one is diffed against the oracle; the patches lower n_left"""
    need(hip_lib, "lvt_amd_track_rgbd16", "lvt_amd_track_rgbd16_async", "lvt_amd_track_rgbd_device")
    q = RSeq(80, {}, (640, 480), 16, patched=True)
    ref = run_host_f32(hip_lib, q, orc=oracle_lib.Oracle(q.prm, 2))
    # the same frames without the patches: more features survive the depth filter (fp32 host entry; the unquantised depth is a different input)
    plain = RSeq(80, {}, (640, 480), 16, device=False)
    base = run_host_f32(hip_lib, plain)
    raw = hip_lib.LvtSystem.create(q.prm, 2)
    raw_poses = [raw.track(*q.world.render_rgbd(i)) for i in range(q.n)]
    assert any(not np.array_equal(raw_poses[i][1], base[i][1]) for i in range(1, q.n)), "quantising the depth changed no pose"
    for i in range(q.n):
        print(f"frame {i}: n_left {ref[i][3]['n_left']} with the patches, {base[i][3]['n_left']} without")
        assert ref[i][3]["n_left"] < base[i][3]["n_left"], i
    # synchronous host u16
    a = hip_lib.LvtSystem.create(q.prm, 2)
    got = []
    odd = np.zeros(q.H * q.W + 9, np.uint16)
    for i in range(q.n):
        u = q.u16[i]
        if i % 2:   # a host plane at a 2-byte-but-not-4-byte aligned address: the staging pull's head and tail elements travel one by one
            k = 1 + ((odd.ctypes.data // 2) % 2)
            u = odd[k:k + q.H * q.W].reshape(q.H, q.W)
            u[:] = q.u16[i]
            assert u.ctypes.data % 4 == 2 and u.flags.c_contiguous
        R, t = a.track(q.gray[i], u, depth_scale=SCALE)
        got.append(record(a, R, t))
    assert a.last_error() == "", a.last_error()
    same_records(got, ref, "host u16 vs host fp32")
    # asynchronous host u16, three frames in flight: poses and states per frame, counters and features after the last one
    b = hip_lib.LvtSystem.create(q.prm, 2)
    res, inflight = [], 0
    for i in range(q.n):
        assert b.track_async(q.gray[i], q.u16[i], depth_scale=SCALE) == 0, b.last_error()
        inflight += 1
        if inflight >= 3:
            res.append(b.wait_status()); inflight -= 1
    while inflight:
        res.append(b.wait_status()); inflight -= 1
    assert b.last_error() == "", b.last_error()
    for i in range(q.n):
        assert np.array_equal(res[i][0], ref[i][0]) and np.array_equal(res[i][1], ref[i][1]) and res[i][2] == ref[i][2], f"async host u16: frame {i}"
    assert b.counts() == ref[-1][3]
    for k in range(3):
        assert np.array_equal(b.features(0)[k], ref[-1][4][k])
    assert b.host_stats()["async_host_frames"] == q.n
    # device u16
    c = hip_lib.LvtSystem.create(q.prm, 2)
    got = []
    for i in range(q.n):
        r = c.track_rgbd_device(q.gray_ptr(i), q.u16_ptr(i), q.H, q.W, q.gpitch, q.u16_pitch(), hip_lib.DEPTH_U16, SCALE)
        assert r is not None, c.last_error()
        got.append(record(c, *r))
    assert c.last_error() == "", c.last_error()
    same_records(got, ref, "device u16 vs host fp32")


def test_uniform_rgbd_batch(hip_lib, oracle_lib):
    """LvtBatch(tum_params, 4, sensor_type=2): seeds 80 - 83, 16 frames, three steps in flight, fp32 for the first 8 steps and 16-bit for the last 8"""
    need(hip_lib, "lvt_amd_batch_track_rgbd_device_async")
    n = 16
    seqs = [RSeq(80 + s, {}, (640, 480), n) for s in range(4)]
    assert len({bytes(q.prm.to_pod()) for q in seqs}) == 1
    batch = hip_lib.LvtBatch(seqs[0].prm, 4, sensor_type=2)
    schedule = [[i] * 4 for i in range(n)]
    fmts = [hip_lib.DEPTH_F32] * 8 + [hip_lib.DEPTH_U16] * 8
    got = batch_run(batch, seqs, schedule, fmts, hip_lib)
    assert batch.last_error() == "", batch.last_error()
    check_against_own_oracles(oracle_lib, batch, seqs, schedule, got)


def test_mixed_rgbd_batch(hip_lib, oracle_lib):
    """distorted / 3 x 2 cells / 320 x 240 / 800 x 600 with a larger radius in one chain; 16 / 16 / 10 / 16 frames, sequence 1 sits step 7 out"""
    need(hip_lib, "lvt_amd_batch_track_rgbd_device_async")
    lens = (16, 16, 10, 16)
    seqs = [RSeq(seed, over, size, m) for (seed, over, size), m in zip(MIXED_CASES, lens)]
    assert seqs[0].prm.k1 != 0 and seqs[1].prm.detection_cell_size == 300 and (seqs[2].W, seqs[3].W) == (320, 800)
    hole, steps = 7, 17
    schedule, nxt = [], [0] * 4
    for k in range(steps):
        which = []
        for s in range(4):
            if nxt[s] < lens[s] and not (s == 1 and k == hole):
                which.append(nxt[s]); nxt[s] += 1
            else:
                which.append(None)
        schedule.append(which)
    assert nxt == list(lens) and schedule[hole][1] is None and schedule[hole + 1][1] == hole
    fmts = [hip_lib.DEPTH_U16 if k % 2 else hip_lib.DEPTH_F32 for k in range(steps)]
    batch = hip_lib.LvtBatch.create_mixed([q.prm for q in seqs], sensor_type=2)
    got, inflight = [], 0
    for k, which in enumerate(schedule):
        if k == hole:                          # drain, so that counts() speaks of step hole - 1 and then of step hole
            while inflight:
                got.append(batch.wait()); inflight -= 1
            before = batch.counts(1)
        assert batch_step(batch, seqs, which, fmts[k], hip_lib) == 0, batch.last_error()
        inflight += 1
        if k == hole:
            got.append(batch.wait()); inflight -= 1
            assert batch.counts(1) == before and before["frame"] == hole - 1, (before, batch.counts(1))
        elif inflight >= 3:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    assert batch.last_error() == "", batch.last_error()
    for k in range(1, steps):                  # an absent step returns the previous step's pose and state
        for s in range(4):
            if schedule[k][s] is None:
                assert np.allclose(got[k][0][s], got[k - 1][0][s], rtol=0, atol=1e-12) and np.allclose(got[k][1][s], got[k - 1][1][s], rtol=0, atol=1e-12), (k, s)
                assert got[k][2][s] == got[k - 1][2][s], (k, s)
    check_against_own_oracles(oracle_lib, batch, seqs, schedule, got)
    assert [batch.counts(s)["frame"] for s in range(4)] == [15, 15, 9, 15]


def test_uniform_equals_mixed_bit_for_bit(hip_lib):
    """three RGB-D sequences under one parameter set through LvtBatch(prm, 3, sensor_type=2) and through the mixed constructor: identical results"""
    need(hip_lib, "lvt_amd_batch_track_rgbd_device_async")
    n = 12
    seqs = [RSeq(86, {}, (320, 240), n, first=2 * s) for s in range(3)]
    schedule = [[i] * 3 for i in range(n)]
    fmts = [hip_lib.DEPTH_F32 if i < 6 else hip_lib.DEPTH_U16 for i in range(n)]
    uni = hip_lib.LvtBatch(seqs[0].prm, 3, sensor_type=2)
    mix = hip_lib.LvtBatch([q.prm for q in seqs], sensor_type=2)
    assert not uni.mixed and mix.mixed
    got_u = batch_run(uni, seqs, schedule, fmts, hip_lib)
    got_m = batch_run(mix, seqs, schedule, fmts, hip_lib)
    assert uni.last_error() == "" and mix.last_error() == ""
    for i in range(n):
        for a, b in zip(got_u[i], got_m[i]):
            assert (a == b).all(), f"frame {i}"
    assert (got_u[-1][2] == 2).all()
    for s in range(3):
        assert uni.counts(s) == mix.counts(s), s


def test_refusals_enqueue_nothing(hip_lib, oracle_lib):
    L = need(hip_lib, "lvt_amd_track_rgbd_device", "lvt_amd_track_rgbd_device_async", "lvt_amd_track_rgbd16", "lvt_amd_track_rgbd16_async",
             "lvt_amd_batch_track_rgbd_device_async")
    F32, U16 = hip_lib.DEPTH_F32, hip_lib.DEPTH_U16
    n = 6
    vp = C.c_void_p

    def refused(h, rc, word=None):
        err = h.last_error()
        assert rc in (-1, None), (rc, err)
        assert err != "" and (word is None or word in err), (word, err)

    # ---- one RGB-D handle
    q = RSeq(86, {}, (320, 240), n)
    one = hip_lib.LvtSystem.create(q.prm, 2)
    orc = oracle_lib.Oracle(q.prm, 2)

    def track_one(i):
        r = one.track_rgbd_device(q.gray_ptr(i), q.u16_ptr(i), q.H, q.W, q.gpitch, q.u16_pitch(), U16, SCALE)
        assert r is not None, one.last_error()
        Ro, to = orc.track_rgbd(q.gray[i], q.f32[i])
        e_t, e_R = pose_errors(r[0], r[1], Ro, to)
        assert e_t <= POSE_TOL and e_R <= POSE_TOL and one.get_state() == orc.status, (i, e_t, e_R)
        co, ch = orc.counts(), one.counts()
        assert not {k: (ch.get(k), v) for k, v in co.items() if ch.get(k) != v}, i
    track_one(0); track_one(1)
    assert one.last_error() == ""
    enq = one.host_stats()["enqueued"]
    assert enq == 2
    g, d32, d16, H, W, gp = q.gray_ptr(2), q.f32_ptr(2), q.u16_ptr(2), q.H, q.W, q.gpitch
    fp, up = q.f32_pitch(), q.u16_pitch()
    R = np.zeros((3, 3)); t = np.zeros(3)
    rp, tp = R.ctypes.data_as(vp), t.ctypes.data_as(vp)
    gh, uh = q.gray[2].ctypes.data_as(vp), q.u16[2].ctypes.data_as(vp)
    dev_async = one.track_rgbd_device_async
    for call, word in (
        (lambda: dev_async(g, 0, H, W, gp, fp, F32), "NULL"),                               # a present frame without a depth plane
        (lambda: dev_async(g, d32, H, W, gp, fp, 7), "unknown depth format"),
        (lambda: dev_async(0, d32, H, W, gp, fp, F32), "NULL"),
        (lambda: dev_async(g, d16, H, W, gp, up, U16, 0.0), "depth_scale"),                 # 16-bit scales that are not finite and > 0
        (lambda: dev_async(g, d32, H + 1, W, gp, fp, F32), "image size"),                   # not this handle's size
        (lambda: dev_async(g, d16, H, W, gp, up, U16, -1.0 / 5000), "depth_scale"),
        (lambda: dev_async(g, d32, H, W, gp + 8, fp, F32), "gray plane"),                   # gray pitch not a multiple of 16
        (lambda: dev_async(g, d16, H, W, gp, up, U16, float("nan")), "depth_scale"),
        (lambda: dev_async(g, d32, H, W - 1, gp, fp, F32), "image size"),
        (lambda: dev_async(g, d16, H, W, gp, up, U16, float("inf")), "depth_scale"),
        (lambda: dev_async(g + 4, d32, H, W, gp, fp, F32), "gray plane"),                   # gray pointer not 16-byte aligned
        (lambda: dev_async(g, d32 + 2, H, W, gp, fp, F32), "depth plane"),                  # fp32 plane at a 2-byte address
        (lambda: dev_async(g, d32, H, W, 16, fp, F32), "gray plane"),                       # gray pitch shorter than the row
        (lambda: dev_async(g, d16 + 1, H, W, gp, up, U16, SCALE), "depth plane"),           # 16-bit plane at an odd address
        (lambda: dev_async(g, d32, H, W, gp, fp, 7), "unknown depth format"),
        (lambda: dev_async(g, d32, H, W, gp, fp + 2, F32), "depth plane"),                  # pitch not a multiple of the element
        (lambda: dev_async(g, d16, H, W, gp, up, U16, 0.0), "depth_scale"),
        (lambda: dev_async(g, d16, H, W, gp, up + 1, U16, SCALE), "depth plane"),
        (lambda: dev_async(g, d32, H, W, gp, fp, -1), "unknown depth format"),
        (lambda: dev_async(g, d32, H, W, gp, 4 * W - 4, F32), "depth plane"),               # pitch shorter than the row
        (lambda: dev_async(g, d32, H + 1, W, gp, fp, F32), "image size"),
        (lambda: dev_async(g, d16, H, W, gp, 2 * W - 2, U16, SCALE), "depth plane"),
        (lambda: one.track_rgbd_device(g, 0, H, W, gp, fp, F32), "NULL"),
        (lambda: one.track_rgbd_device(g, d16, H, W, gp, up, U16, 0.0), "depth_scale"),
        (lambda: L.lvt_amd_track_rgbd16(one._h, gh, None, float(SCALE), H, W, rp, tp), "lvt_amd_track_rgbd16: NULL"),
        (lambda: L.lvt_amd_track_rgbd16(one._h, gh, uh, 0.0, H, W, rp, tp), "lvt_amd_track_rgbd16: depth_scale"),
        (lambda: L.lvt_amd_track_rgbd16(one._h, gh, uh, float(SCALE), H, W + 1, rp, tp), "lvt_amd_track_rgbd16: image size"),
        (lambda: L.lvt_amd_track_rgbd16_async(one._h, gh, None, float(SCALE), H, W), "lvt_amd_track_rgbd16_async: NULL"),
        (lambda: L.lvt_amd_track_rgbd16_async(one._h, gh, uh, float("nan"), H, W), "lvt_amd_track_rgbd16_async: depth_scale"),
        (lambda: L.lvt_amd_track_rgbd16_async(one._h, gh, uh, float(SCALE), H - 1, W), "lvt_amd_track_rgbd16_async: image size"),
        (lambda: L.lvt_amd_batch_track_rgbd_device_async(one._h, None, None, None, None, None, None, F32, 1.0), "NULL argument"),
    ):
        refused(one, call(), word)
        assert one.host_stats()["enqueued"] == enq, word
    assert not R.any() and not t.any()
    # the stereo device calls on an RGB-D handle: an error string instead of a frame without a depth plane
    one.track_device_async(g, g, H, W, gp)
    refused(one, None, "RGB-D")
    Rt = one.track_device(g, g, H, W, gp)
    refused(one, None, "RGB-D")
    assert not Rt[0].any() and not Rt[1].any()
    assert one.host_stats()["enqueued"] == enq
    for i in range(2, n):                      # the next valid frames track as if nothing had happened
        track_one(i)
    assert orc.status == 2

    # ---- an RGB-D batch (mixed: two sizes)
    seqs = [q, RSeq(80, {}, (640, 480), n)]
    batch = hip_lib.LvtBatch.create_mixed([s.prm for s in seqs], sensor_type=2)
    schedule = [[i, i] for i in range(n)]
    fmts = [U16, F32] * (n // 2)
    got = batch_run(batch, seqs, schedule[:2], fmts[:2], hip_lib)
    assert batch.last_error() == ""
    enq = batch.host_stats()["enqueued"]
    assert enq == 2
    G = [s.gray_ptr(2) for s in seqs]; D = [s.f32_ptr(2) for s in seqs]; D16 = [s.u16_ptr(2) for s in seqs]
    Hs, Ws, GP = [s.H for s in seqs], [s.W for s in seqs], [s.gpitch for s in seqs]
    FP, UP = [s.f32_pitch() for s in seqs], [s.u16_pitch() for s in seqs]
    bt = batch.track_rgbd_device_async
    for call, word in (
        (lambda: bt(G, [D[0], None], Hs, Ws, GP, FP, F32), "sequence 1: NULL"),                      # present, no depth plane
        (lambda: bt(G, D, Hs, Ws, GP, FP, 2), "unknown depth format"),
        (lambda: bt(G, D16, Hs, Ws, GP, UP, U16, 0.0), "depth_scale"),
        (lambda: bt(G, D, Hs, [Ws[0], Ws[0]], GP, FP, F32), "sequence 1: image size"),               # sequence 1 handed sequence 0's width
        (lambda: bt(G, D16, Hs, Ws, GP, UP, U16, float("inf")), "depth_scale"),
        (lambda: bt(G, D, [Hs[0] + 1, Hs[1]], Ws, GP, FP, F32), "sequence 0: image size"),
        (lambda: bt(G, D, Hs, Ws, [GP[0], GP[1] + 8], FP, F32), "sequence 1: gray plane"),
        (lambda: bt(G, D, Hs, Ws, GP, [FP[0] + 2, FP[1]], F32), "sequence 0: depth plane"),
        (lambda: bt(G, [D16[0], D16[1] + 1], Hs, Ws, GP, UP, U16, SCALE), "sequence 1: depth plane"),
        (lambda: bt([None, None], [None, None], Hs, Ws, GP, FP, F32), "no sequence"),
        (lambda: L.lvt_amd_track_rgbd_device_async(batch._h, vp(G[0]), GP[0], vp(D[0]), FP[0], F32, 1.0, Hs[0], Ws[0]), "a batch handle"),
        (lambda: batch.track_device_async_mixed(G, G, Hs, Ws, GP), "RGB-D"),                          # the stereo batch call
    ):
        refused(batch, call(), word)
        assert batch.host_stats()["enqueued"] == enq, word
    got += batch_run(batch, seqs, schedule[2:], fmts[2:], hip_lib)
    check_against_own_oracles(oracle_lib, batch, seqs, schedule, got)
    uni = hip_lib.LvtBatch(q.prm, 2, sensor_type=2)
    uni.track_device_async([g, g], [g, g], H, W, gp)                                                   # the uniform stereo call on a uniform RGB-D batch
    refused(uni, None, "RGB-D")
    assert uni.host_stats()["enqueued"] == 0
    uq = [q, RSeq(86, {}, (320, 240), n, first=3)]
    got = batch_run(uni, uq, schedule, fmts, hip_lib)
    check_against_own_oracles(oracle_lib, uni, uq, schedule, got)

    # ---- the RGB-D calls on stereo handles: a batch, a solo handle, a pooled handle
    world, sprm, _ = make_case("kitti", 32, 1.0, None, size=(620, 188))
    import torch
    sn = 4
    sp = ((world.W + 63) // 64) * 64
    sdev = torch.zeros((sn + 2, 2, world.H, sp), dtype=torch.uint8, device="cuda")
    sfr = [world.render_stereo(i) for i in range(sn + 2)]
    for i, (a, b) in enumerate(sfr):
        sdev[i, 0, :, :world.W] = torch.from_numpy(a).cuda(); sdev[i, 1, :, :world.W] = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    fake_depth = torch.ones((world.H, world.W), dtype=torch.float32, device="cuda")
    sb = hip_lib.LvtBatch(sprm, 2)
    rc = sb.track_rgbd_device_async([sdev[0, 0].data_ptr()] * 2, [fake_depth.data_ptr()] * 2, world.H, world.W, sp, 4 * world.W, F32)
    refused(sb, rc, "stereo")
    assert sb.host_stats()["enqueued"] == 0
    res, inflight = [], 0
    for i in range(sn):
        sb.track_device_async([sdev[i, 0].data_ptr(), sdev[i + 2, 0].data_ptr()], [sdev[i, 1].data_ptr(), sdev[i + 2, 1].data_ptr()], world.H, world.W, sp)
        res.append(sb.wait())
    for s in range(2):
        so = oracle_lib.Oracle(sprm, 1)
        for i in range(sn):
            Ro, to = so.track(*sfr[i + 2 * s])
            e_t, e_R = pose_errors(res[i][0][s], res[i][1][s], Ro, to)
            assert e_t <= POSE_TOL and e_R <= POSE_TOL and res[i][2][s] == so.status, (s, i, e_t, e_R)
        co, ch = so.counts(), sb.counts(s)
        assert not {k: (ch.get(k), v) for k, v in co.items() if ch.get(k) != v}, s
    for pooled in (False, True):
        st = hip_lib.LvtSystem.create(sprm, 1, pooled=pooled)
        word = "pooled" if pooled else "stereo"
        refused(st, st.track_rgbd_device_async(sdev[0, 0].data_ptr(), fake_depth.data_ptr(), world.H, world.W, sp, 4 * world.W, F32), word)
        refused(st, st.track_rgbd_device(sdev[0, 0].data_ptr(), fake_depth.data_ptr(), world.H, world.W, sp, 4 * world.W, F32), word)
        z16 = np.zeros((world.H, world.W), np.uint16)
        refused(st, L.lvt_amd_track_rgbd16(st._h, sfr[0][0].ctypes.data_as(vp), z16.ctypes.data_as(vp), float(SCALE), world.H, world.W, rp, tp), word)
        refused(st, L.lvt_amd_track_rgbd16_async(st._h, sfr[0][0].ctypes.data_as(vp), z16.ctypes.data_as(vp), float(SCALE), world.H, world.W), word)
        assert st.host_stats()["enqueued"] == 0
        so = oracle_lib.Oracle(sprm, 1)
        for i in range(3):
            Rh, th = st.track(*sfr[i])
            Ro, to = so.track(*sfr[i])
            e_t, e_R = pose_errors(Rh, th, Ro, to)
            assert e_t <= POSE_TOL and e_R <= POSE_TOL and st.get_state() == so.status, (pooled, i, e_t, e_R)
        st.close()
