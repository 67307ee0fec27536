"""One handle, every way a frame can enter it.  The entry points share the ring of per-frame input records (RING slots); here they alternate with a
period of five -- coprime with RING = 8 -- over 2 RING + 3 frames, so every slot is filled by one kind of call and, RING frames later, by another.  A
field that one kind sets and the next leaves alone would reach the kernels stale; the run is held to the oracle frame by frame."""
import numpy as np
import pytest

from parity_util import make_case, pose_errors, diff_frame, POSE_TOL
from rgbd_util import quantise, SCALE

pytestmark = pytest.mark.gpu

RING = 8   # lvt_host.hip
N = 2 * RING + 3


def _pinned(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy()


def _interleave(hip, n, submit, sync_kinds):
    """frame i enters through kind i % 5; the synchronous kinds return (R, t), the others are left in flight -- three of them at the most -- and collected
    before the next synchronous call.  Returns [(R, t, state)] per frame."""
    got, inflight = [], 0
    for i in range(n):
        kind = i % 5
        if kind in sync_kinds:
            while inflight:
                got.append(hip.wait_status()); inflight -= 1
            R, t = submit(kind, i)
            got.append((R, t, hip.get_state()))
        else:
            assert submit(kind, i) in (0, None), hip.last_error()
            inflight += 1
            if inflight > 3:
                got.append(hip.wait_status()); inflight -= 1
    while inflight:
        got.append(hip.wait_status()); inflight -= 1
    assert len(got) == n
    return got


def _hold_to_the_oracle(hip, orc, got, expected):
    for i, (Ro, to, so) in enumerate(expected):
        Rh, th, st = got[i]
        e_t, e_R = pose_errors(Rh, th, Ro, to)
        print(f"frame {i} (kind {i % 5}): e_t {e_t:.2e} e_R {e_R:.2e} state {st} / {so}")
        assert e_t <= POSE_TOL and e_R <= POSE_TOL and st == so, f"frame {i} (kind {i % 5}): e_t {e_t:.2e} e_R {e_R:.2e} state {st} / {so}"
    msgs = diff_frame(hip, orc)
    assert not msgs, msgs[:6]
    assert hip.last_error() == "", hip.last_error()
    assert hip.host_stats()["enqueued"] == len(expected), hip.host_stats()


def test_stereo_entry_points_interleaved_on_one_handle(hip_lib, oracle_lib):
    """lvt_track, lvt_track_with_external_corners, lvt_amd_track_async (pageable, then page-locked buffers) and lvt_amd_track_device_async in turn"""
    import torch
    O = oracle_lib
    world, prm, _ = make_case("kitti", 8, 0.5)
    frames = [world.render_stereo(i) for i in range(N)]
    pitch = ((world.W + 63) // 64) * 64
    dev = torch.zeros((N, 2, world.H, pitch), dtype=torch.uint8, device="cuda")
    keep, corners = {}, {}
    rng = np.random.default_rng(5)
    for i, (a, b) in enumerate(frames):
        if i % 5 == 1:   # the lists of test_external_corners
            xl, _, _, _ = O.compute_features(a, prm)
            xr, _, _, _ = O.compute_features(b, prm)
            cl = xl.astype(np.float64); cr = xr.astype(np.float64)
            cl[::7] += rng.uniform(-0.5, 0.5, size=cl[::7].shape)
            cr[::5] += 0.5
            corners[i] = (np.vstack([cl, [[3.0, 3.0], [world.W - 28.5, world.H - 28.5], [27.5, 27.5]]]), cr)
        elif i % 5 == 2:
            keep[i] = (np.ascontiguousarray(a), np.ascontiguousarray(b))
        elif i % 5 == 3:
            keep[i] = (_pinned(a), _pinned(b))
        elif i % 5 == 4:
            dev[i, 0, :, :world.W] = torch.from_numpy(a).cuda(); dev[i, 1, :, :world.W] = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    hip = hip_lib.LvtSystem.create(prm, 1)
    orc = O.Oracle(prm, 1)

    def submit(kind, i):
        if kind == 0:
            return hip.track(*frames[i])
        if kind == 1:
            return hip.track_with_external_corners(*frames[i], *corners[i])
        if kind in (2, 3):
            return hip.track_async(*keep[i])
        return hip.track_device_async(dev[i, 0].data_ptr(), dev[i, 1].data_ptr(), world.H, world.W, pitch)
    got = _interleave(hip, N, submit, (0, 1))
    expected = []
    for i, (a, b) in enumerate(frames):
        Ro, to = orc.track_with_external_corners(a, b, *corners[i]) if i % 5 == 1 else orc.track(a, b)
        expected.append((Ro, to, orc.status))
    _hold_to_the_oracle(hip, orc, got, expected)
    hs = hip.host_stats()
    assert hs["planes_in_place"] > 0 and hs["planes_staged"] > 0 and hs["async_host_frames"] == len(keep), hs


def test_rgbd_entry_points_interleaved_on_one_handle(hip_lib, oracle_lib):
    """lvt_amd_track_rgbd, lvt_amd_track_rgbd16, lvt_amd_track_rgbd_async, lvt_amd_track_rgbd16_async and lvt_amd_track_rgbd_device_async in turn; the
    depth is quantised to 16 bits for every frame and the oracle (and every fp32 entry) gets u * s, as in test_gpu_rgbd_batch.test_u16_equals_f32"""
    import torch
    world, prm, sensor = make_case("tum", 4, 0.5)
    assert sensor == 2
    gray, u16, f32 = [], [], []
    for i in range(N):
        g, d = world.render_rgbd(i)
        u = quantise(d)
        assert int(u.max()) < 65535
        gray.append(np.ascontiguousarray(g)); u16.append(u); f32.append(u.astype(np.float32) * SCALE)
    gpitch = ((world.W + 63) // 64) * 64
    d_gray = torch.zeros((N, world.H, gpitch), dtype=torch.uint8, device="cuda")
    d_f32 = torch.zeros((N, world.H, world.W + 12), dtype=torch.float32, device="cuda")   # (rows padded by 12 elements)
    for i in range(4, N, 5):
        d_gray[i, :, :world.W] = torch.from_numpy(gray[i]).cuda(); d_f32[i, :, :world.W] = torch.from_numpy(f32[i]).cuda()
    torch.cuda.synchronize()
    hip = hip_lib.LvtSystem.create(prm, 2)
    orc = oracle_lib.Oracle(prm, 2)

    def submit(kind, i):
        if kind == 0:
            return hip.track(gray[i], f32[i])
        if kind == 1:
            return hip.track(gray[i], u16[i], depth_scale=SCALE)
        if kind == 2:
            return hip.track_async(gray[i], f32[i])
        if kind == 3:
            return hip.track_async(gray[i], u16[i], depth_scale=SCALE)
        return hip.track_rgbd_device_async(d_gray[i].data_ptr(), d_f32[i].data_ptr(), world.H, world.W, gpitch, 4 * (world.W + 12), hip_lib.DEPTH_F32)
    got = _interleave(hip, N, submit, (0, 1))
    expected = []
    for i in range(N):
        Ro, to = orc.track_rgbd(gray[i], f32[i])
        expected.append((Ro, to, orc.status))
    _hold_to_the_oracle(hip, orc, got, expected)
