"""Unregistered depth on the GPU (lvt_amd_set_depth_camera, k_depth_clear / k_depth_register): the stage alone against the numpy restatement bit for bit,
the identity camera against no camera, the two 320 x 240 sequences of test_depth_registration.py through every RGB-D entry point against the oracle fed the
numpy-registered planes, a mixed batch, the launch accounting and every refusal.  A last-bit difference against numpy is a finding to trace to its operation,
never a tolerance."""
import copy
import ctypes as C

import numpy as np
import pytest

import depth_reg_util as D
from parity_util import diff_frame, pose_errors, POSE_TOL
from rgbd_util import SCALE, need, record, same_records, check_against_own_oracles

pytestmark = pytest.mark.gpu
F = np.float32
NEW = ("lvt_amd_set_depth_camera", "lvt_amd_batch_set_depth_camera", "lvt_amd_get_depth_camera", "lvt_amd_register_depth_device")
TUM_DISTORTION = {"k1": 0.262383, "k2": -0.953104, "p1": -0.005358, "p2": 0.002628, "k3": 1.163314}   # config_tum1.yaml


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the stage alone ---------------------------------------------------------------------------------------------------------------------------
def dev_plane(a, pad_el=0, odd=False, fill=0):
    """a host plane in HBM with rows padded by pad_el elements; odd: a 16-bit plane at an address that is 2 but not 0 modulo 4.  (tensor, pointer, pitch in bytes)"""
    import torch
    h, w = a.shape
    tt = {np.dtype(np.float32): torch.float32, np.dtype(np.uint16): torch.int16}[a.dtype]
    flat = torch.full((h * (w + pad_el) + 2,), fill, dtype=tt, device="cuda")
    off = 1 if odd else 0
    v = flat[off: off + h * (w + pad_el)].view(h, w + pad_el)
    v[:, :w] = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    ptr = flat.data_ptr() + off * a.itemsize
    if odd:
        assert a.itemsize == 2 and ptr % 4 == 2
    return flat, ptr, (w + pad_el) * a.itemsize


def run_stage(hip_lib, cam, prm, depth, scale=None, pad_el=0, odd=False, out_pad=0):
    """lvt_amd_register_depth_device on a copy of `depth` in HBM; the whole destination (img_height x (img_width + out_pad)), which starts out as garbage"""
    import torch
    keep, ptr, pitch = dev_plane(depth, pad_el, odd, fill=7)
    H, P = prm.img_height, prm.img_width + out_pad
    out = torch.full((H, P), -3.0, dtype=torch.float32, device="cuda")
    fmt = hip_lib.DEPTH_U16 if depth.dtype == np.uint16 else hip_lib.DEPTH_F32
    rc = hip_lib.register_depth_device(cam, prm, ptr, pitch, fmt, 0.0 if scale is None else float(scale), out.data_ptr(), 4 * P, 0)
    assert rc == 0
    torch.cuda.synchronize()
    del keep
    return out.cpu().numpy()


def check_stage(hip_lib, cam, prm, depth, scale=None, **kw):
    out_pad = kw.get("out_pad", 0)
    got = run_stage(hip_lib, cam, prm, depth, scale, **kw)
    want = D.register(cam, prm, depth, scale, pitch=prm.img_width + out_pad)
    bad = np.argwhere(bits(got) != bits(want))
    assert not len(bad), f"{len(bad)} words differ, first (row, column) {tuple(bad[0])}: gpu {got[tuple(bad[0])]!r} numpy {want[tuple(bad[0])]!r}"
    if out_pad:
        assert np.all(np.isposinf(got[:, prm.img_width:]))
    return got


def synth_depth(w, h, seed, lo=0.4, hi=4.5):
    """a piecewise-smooth depth image with steps (occlusions) and holes"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    d = 2.0 + 0.8 * np.sin(x / 9.0 + seed) + 0.5 * np.cos(y / 7.0)
    for _ in range(6):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        d[y0: y0 + int(rng.integers(2, h // 2 + 3)), x0: x0 + int(rng.integers(2, w // 2 + 3))] = rng.uniform(lo, hi)
    d[rng.random((h, w)) < 0.03] = 0.0
    return np.clip(d, 0, hi).astype(F)


def small_prm(hip_lib, w, h, **kw):
    p = hip_lib.tum_params(width=w, height=h, fx=517.306408 * w / 640, fy=516.469215 * w / 640, cx=318.64304 * w / 640, cy=255.313989 * h / 480)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def scaled_camera(prm, w, h, R=None, t=None):
    sx, sy = w / prm.img_width, h / prm.img_height
    return D.make_camera(w, h, prm.fx * sx, prm.fy * sy, prm.cx * sx, prm.cy * sy, R, t)


def test_stage_identity_camera(hip_lib):
    need(hip_lib, *NEW)
    prm = small_prm(hip_lib, 80, 60)
    d = synth_depth(80, 60, 1)
    d[5, 6], d[9, 2], d[11, 11] = np.nan, -1.0, np.inf
    got = check_stage(hip_lib, D.identity_camera(prm), prm, d)
    assert np.array_equal(bits(got), bits(np.where((d > 0) & np.isfinite(d), d, F(np.inf)).astype(F)))


@pytest.mark.parametrize("dsize,csize", [((80, 60), (160, 120)), ((160, 120), (80, 60))])
def test_stage_other_sizes(hip_lib, dsize, csize):
    """80 x 60 -> 160 x 120 (footprints of 2 - 3 px) and 160 x 120 -> 80 x 60 (<= 1 px, most pixels taking several depth pixels)"""
    prm = small_prm(hip_lib, *csize)
    cam = scaled_camera(prm, *dsize, t=(0.05, 0, 0))
    d = synth_depth(*dsize, 2)
    got = check_stage(hip_lib, cam, prm, d)
    _, span = D.register_numpy(cam, prm, d)
    print("largest footprint", span, "holes", D.holes(got, csize[0]))
    assert (2 <= max(span) <= 3) if dsize[0] < csize[0] else max(span) <= 1


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_stage_rotated_camera(hip_lib, axis):
    """7 degrees about each axis and 5 cm to the side"""
    prm = small_prm(hip_lib, 80, 60)
    check_stage(hip_lib, scaled_camera(prm, 80, 60, D.rot(axis, 7.0), (0.05, 0.0, 0.0)), prm, synth_depth(80, 60, 3 + axis))


def test_stage_distorted_colour_camera(hip_lib):
    """the colour side with config_tum1.yaml's distortion coefficients"""
    prm = small_prm(hip_lib, 160, 120, **TUM_DISTORTION)
    got = check_stage(hip_lib, D.offset_camera(prm, 160, 120), prm, synth_depth(160, 120, 8))
    plain = small_prm(hip_lib, 160, 120)
    assert not np.array_equal(bits(got), bits(D.register(D.offset_camera(plain, 160, 120), plain, synth_depth(160, 120, 8))))   # (the coefficients matter)


def test_stage_formats_pitches_and_padding(hip_lib):
    """a 16-bit source at a 2-byte-but-not-4-byte aligned address with a padded pitch; an fp32 source with a padded pitch; a destination pitch larger than the
    row, whose padding must come out +inf"""
    prm = small_prm(hip_lib, 80, 60)
    cam = D.offset_camera(prm, 72, 50)
    d = synth_depth(72, 50, 9)
    u = np.clip(np.rint(d.astype(np.float64) * 5000), 0, 65535).astype(np.uint16)
    a = check_stage(hip_lib, cam, prm, u, SCALE, pad_el=6, odd=True, out_pad=16)
    b = check_stage(hip_lib, cam, prm, u.astype(F) * SCALE, pad_el=12, out_pad=16)
    assert np.array_equal(bits(a), bits(b))   # (a 16-bit plane registers like its fp32 conversion)
    check_stage(hip_lib, cam, prm, d, out_pad=3)   # (a destination whose rows are not 16-byte multiples)


@pytest.mark.parametrize("name", ["invalid depths", "nearer wins", "behind the camera", "edges"])
def test_stage_constructed_case(hip_lib, name):
    cases, prm = D.constructed_case()
    cam, d, want = cases[name]
    got = check_stage(hip_lib, cam, prm, d)
    assert np.array_equal(bits(got), bits(want)), (got, want)


@pytest.mark.parametrize("axis", [0, 1])
def test_stage_footprint_cap(hip_lib, axis):
    for diff in (15, 16):
        cam, prm, d, want = D.span_case(diff, axis)
        got = check_stage(hip_lib, cam, prm, d)
        assert np.array_equal(bits(got), bits(want)), (diff, np.argwhere(np.isfinite(got)))


def test_stage_degenerate_planes(hip_lib):
    """an all-zero plane gives an all-+inf plane; 1 x 1 and one-row planes"""
    prm = small_prm(hip_lib, 80, 60)
    got = check_stage(hip_lib, D.identity_camera(prm), prm, np.zeros((60, 80), F))
    assert np.all(np.isposinf(got))
    one = D.make_camera(1, 1, 2.0, 2.0, 0.0, 0.0, None, (0.1, 0.05, 0))      # one pixel 1 / 2 wide in angle: a footprint of many colour pixels
    got = check_stage(hip_lib, one, small_prm(hip_lib, 8, 6, fx=20.0, fy=20.0, cx=3.2, cy=2.1), np.full((1, 1), 1.5, F))
    assert np.isfinite(got).sum() > 1
    p1 = small_prm(hip_lib, 1, 1, fx=1.0, fy=1.0, cx=0.0, cy=0.0)
    got = check_stage(hip_lib, D.identity_camera(p1), p1, np.full((1, 1), 0.75, F))
    assert got[0, 0] == F(0.75)
    row = D.make_camera(80, 1, prm.fx, prm.fy, prm.cx, 0.0, None, (0.0, 0.0, 0.0))
    got = check_stage(hip_lib, row, prm, synth_depth(80, 1, 4))
    assert np.isfinite(got).any(axis=1).sum() == 1     # (the row lands on one row of the colour image, around cy)


def test_stage_many_to_one(hip_lib):
    """many depth pixels on one colour pixel: a 64 x 64 depth plane whose focal length is 8 times the colour camera's, into a 16 x 16 colour image -- 64 depth
    pixels per colour pixel, of which the one whose footprint holds the pixel's centre writes --, and the heaviest pile-up the definition allows at these sizes.
    A depth pixel writes a colour pixel at most once and footprints of one depth tile the image, so pixels only pile up through depth: here 32 pixels of two
    depth columns, rows 0 - 31, each in another wavefront and four to a workgroup, carry the depth that puts their 15 x 15 footprint on rows 1 - 15 of the colour
    image (v = 15 (j - 32) + 15 t_y / z + 8 with z = t_y / (32 - j)): every pixel there takes 32 atomics from eight workgroups, and the minimum must be exact --
    once with the nearest pixel in the first workgroup of the eight, once, mirrored, in the last"""
    prm = small_prm(hip_lib, 16, 16, fx=8.0, fy=8.0, cx=8.0, cy=8.0)
    rng = np.random.default_rng(12)
    d = rng.uniform(0.5, 4.0, (64, 64)).astype(F)
    got = check_stage(hip_lib, D.make_camera(64, 64, 64.0, 64.0, 32.0, 32.0), prm, d)    # u = (i - 32) / 8 + 8: the centre 8 x 8 of the colour image
    assert np.isfinite(got[4:12, 4:12]).all() and np.isposinf(got[:4]).all()
    prm = small_prm(hip_lib, 16, 16, fx=15.0, fy=15.0, cx=8.0, cy=8.0)
    cam = D.make_camera(64, 64, 1.0, 1.0, 32.0, 32.0, None, (0.0, 16.0, 0.0))
    d = rng.uniform(0.5, 4.0, (64, 64)).astype(F)
    d[:32, :] = (16.0 / (32 - np.arange(32, dtype=np.float64)))[:, None].astype(F)
    counts = np.zeros(256, np.int64)
    D.register_numpy(cam, prm, d, counts=counts)
    counts = counts.reshape(16, 16)
    print("writes per colour pixel, rows 1 - 15:", counts[1:].min(), "-", counts[1:].max())
    assert counts[1:].min() >= 32
    got = check_stage(hip_lib, cam, prm, d)
    assert np.all(got[1:] == F(0.5))            # (the nearest pixel is row 0: the FIRST workgroup's)
    # ... and mirrored, so that the winner arrives from the LAST workgroup: t_y = -16, rows 33 - 63 with z = 16 / (j - 32), the nearest in row 63
    cam = D.make_camera(64, 64, 1.0, 1.0, 32.0, 32.0, None, (0.0, -16.0, 0.0))
    d = rng.uniform(0.5, 4.0, (64, 64)).astype(F)
    d[33:, :] = (16.0 / (np.arange(33, 64, dtype=np.float64) - 32))[:, None].astype(F)
    counts = np.zeros(256, np.int64)
    D.register_numpy(cam, prm, d, counts=counts)
    assert counts.reshape(16, 16)[1:].min() >= 31
    got = check_stage(hip_lib, cam, prm, d)
    assert np.all(got[1:] == F(16.0 / 31.0))


# ---- 2. inside the tracker ------------------------------------------------------------------------------------------------------------------------
class Planes:
    """a sequence's planes in HBM: gray, and the sensor's depth as 16-bit (odd address, padded pitch) and fp32 (padded pitch)"""

    def __init__(self, q):
        import torch
        self.q = q
        self.gpitch = ((q.W + 63) // 64) * 64
        self.d_gray = torch.zeros((q.n, q.H, self.gpitch), dtype=torch.uint8, device="cuda")
        for i in range(q.n):
            self.d_gray[i, :, :q.W] = torch.from_numpy(q.gray[i]).cuda()
        self.u16 = [dev_plane(u, 6, odd=True, fill=15000) for u in q.s_u16]
        self.f32 = [dev_plane(f, 12, fill=3) for f in q.s_f32]
        torch.cuda.synchronize()

    def gray(self, i):
        return self.d_gray[i].data_ptr()

    def depth(self, i, fmt):
        _, ptr, pitch = (self.u16 if fmt == 1 else self.f32)[i]
        return ptr, pitch


_PLANES = {}


def planes(which):
    if which not in _PLANES:
        _PLANES[which] = Planes(D.sequence(which))
    return _PLANES[which]


def system_with_camera(hip_lib, q):
    sys_ = hip_lib.LvtSystem.create(q.prm, 2)
    assert sys_.set_depth_camera(q.cam) == 0, sys_.last_error()
    return sys_


def held_to_oracle(sys_, orc, R, t, Ro, to, i):
    msgs = diff_frame(sys_, orc)
    e_t, e_R = pose_errors(R, t, Ro, to)
    print(f"frame {i}: e_t {e_t:.2e} e_R {e_R:.2e} n_left {sys_.counts()['n_left']} state {orc.status}")
    assert not msgs, f"frame {i}: {msgs[:6]}"
    assert e_t <= POSE_TOL and e_R <= POSE_TOL, f"frame {i}: {e_t:.2e} {e_R:.2e}"
    assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"


def registered_plane_equals_numpy(sys_, q, i):
    got = sys_.plane(0, 4)
    assert got.dtype == F and got.shape[0] == q.H and got.shape[1] >= q.W
    want = D.register(q.cam, q.prm, q.s_u16[i], SCALE, pitch=got.shape[1])
    bad = np.argwhere(bits(got) != bits(want))
    assert not len(bad), f"frame {i}: {len(bad)} words of the registered plane differ from numpy, first {tuple(bad[0])}"


def test_identity_camera_equals_no_camera(hip_lib):
    """an RGB-D handle with the identity camera produces, over 12 frames, records byte-identical to a handle without one"""
    need(hip_lib, *NEW)
    q = D.sequence("plain")
    runs = []
    for with_cam in (False, True):
        sys_ = hip_lib.LvtSystem.create(q.prm, 2)
        if with_cam:
            assert sys_.set_depth_camera(D.identity_camera(q.prm)) == 0, sys_.last_error()
        out = []
        for i in range(q.n):
            R, t = sys_.track(q.gray[i], q.f32[i])
            out.append(record(sys_, R, t))
        assert sys_.last_error() == "", sys_.last_error()
        assert (sys_.plane(0, 4).size > 0) == with_cam
        runs.append(out)
        sys_.close()
    assert runs[0][-1][2] == 2
    same_records(runs[0], runs[1], "identity camera / no camera")


@pytest.mark.parametrize("which", ["same", "half"])
@pytest.mark.parametrize("route", ["rgbd16", "rgbd_async", "device", "device_async"])
def test_sequences_against_the_oracle(hip_lib, oracle_lib, which, route):
    """lvt_amd_track_rgbd16, lvt_amd_track_rgbd_async (three in flight), lvt_amd_track_rgbd_device and _device_async take the sensor's planes; every frame is held
    to the oracle fed the numpy-registered plane, and the registered plane of each synchronous frame equals numpy's bit for bit.  The synchronous routes apply
    diff_frame to every frame.  With three frames in flight the introspection calls answer for the last collected frame only and would drain the pipeline: there
    every frame is held by pose and state as it is collected, and diff_frame -- features, matches, map, staged points, counters: all of which carry the whole
    history -- is applied once the handle is drained, behind the last frame"""
    need(hip_lib, *NEW)
    q = D.sequence(which)
    orc = oracle_lib.Oracle(q.prm, 2)
    sys_ = system_with_camera(hip_lib, q)
    if route in ("rgbd16", "device"):
        P = planes(which) if route == "device" else None
        for i in range(q.n):
            if route == "rgbd16":
                R, t = sys_.track(q.gray[i], q.s_u16[i], depth_scale=SCALE)
            else:
                fmt = hip_lib.DEPTH_U16 if i % 2 else hip_lib.DEPTH_F32
                ptr, pitch = P.depth(i, fmt)
                got = sys_.track_rgbd_device(P.gray(i), ptr, q.H, q.W, P.gpitch, pitch, fmt, SCALE)
                assert got is not None, sys_.last_error()
                R, t = got
            Ro, to = orc.track_rgbd(q.gray[i], q.f32[i])
            held_to_oracle(sys_, orc, R, t, Ro, to, i)
            registered_plane_equals_numpy(sys_, q, i)
    else:
        P = planes(which) if route == "device_async" else None
        inflight = []

        def collect():
            i = inflight.pop(0)
            R, t, st = sys_.wait_status()
            Ro, to = orc.track_rgbd(q.gray[i], q.f32[i])
            e_t, e_R = pose_errors(R, t, Ro, to)
            assert st == orc.status == 2 and e_t <= POSE_TOL and e_R <= POSE_TOL, f"frame {i}: state {st} / {orc.status}, {e_t:.2e} {e_R:.2e}"
            if not inflight:   # (the handle is drained: the introspection calls answer for this frame)
                msgs = diff_frame(sys_, orc)
                assert not msgs, f"frame {i}: {msgs[:6]}"
        for i in range(q.n):
            if route == "rgbd_async":
                assert sys_.track_async(q.gray[i], q.s_f32[i]) == 0, sys_.last_error()
            else:
                fmt = hip_lib.DEPTH_F32 if i % 2 else hip_lib.DEPTH_U16
                ptr, pitch = P.depth(i, fmt)
                assert sys_.track_rgbd_device_async(P.gray(i), ptr, q.H, q.W, P.gpitch, pitch, fmt, SCALE) == 0, sys_.last_error()
            inflight.append(i)
            if len(inflight) == 3:
                collect()
        while inflight:
            collect()
        registered_plane_equals_numpy(sys_, q, q.n - 1)
    assert sys_.last_error() == "", sys_.last_error()
    sys_.close()


def test_depth_camera_larger_than_the_image(hip_lib, oracle_lib):
    """a 400 x 300 depth camera on a 320 x 240 image: the host entry points stage, pull and hold planes larger than the ones the handle was created with --
    first frames registered (no camera yet), then the camera, synchronous and asynchronous, 16-bit and fp32"""
    q, plain = D.sequence("big", 6), D.sequence("plain")
    sys_, orc = hip_lib.LvtSystem.create(q.prm, 2), oracle_lib.Oracle(q.prm, 2)
    for i in range(2):
        assert sys_.track_async(plain.gray[i], plain.f32[i]) == 0, sys_.last_error()
        R, t, st = sys_.wait_status()
        Ro, to = orc.track_rgbd(plain.gray[i], plain.f32[i])
        held_to_oracle(sys_, orc, R, t, Ro, to, i)
    assert sys_.set_depth_camera(q.cam) == 0, sys_.last_error()
    for call in (sys_.track, sys_.track_async):   # (the binding knows the array's shape, the C-ABI does not: an image-sized plane would be read past its end)
        with pytest.raises(ValueError):
            call(plain.gray[2], plain.f32[2])
    for i in range(2, 6):
        if i < 4:
            R, t = sys_.track(q.gray[i], q.s_u16[i], depth_scale=SCALE) if i == 2 else sys_.track(q.gray[i], q.s_f32[i])
        else:
            assert (sys_.track_async(q.gray[i], q.s_u16[i], depth_scale=SCALE) if i == 4 else sys_.track_async(q.gray[i], q.s_f32[i])) == 0, sys_.last_error()
            R, t, st = sys_.wait_status()
        Ro, to = orc.track_rgbd(q.gray[i], q.f32[i])
        held_to_oracle(sys_, orc, R, t, Ro, to, i)
        registered_plane_equals_numpy(sys_, q, i)
    assert sys_.last_error() == "", sys_.last_error()
    sys_.close()


class _BatchSeq:
    """what rgbd_util.check_against_own_oracles reads of a sequence"""

    def __init__(self, q):
        self.prm, self.gray, self.f32 = q.prm, q.gray, q.f32


def test_mixed_batch(hip_lib, oracle_lib):
    """three sequences: a same-size depth camera, a half-size one, none; sequence 1 sits steps out and the depth format changes between steps; each sequence is
    held to its own oracle"""
    need(hip_lib, *NEW)
    names = ("same", "half", "plain")
    seqs = [D.sequence(w) for w in names]
    P = [planes(w) for w in names]
    batch = hip_lib.LvtBatch.create_mixed([q.prm for q in seqs], 2)
    for s, q in enumerate(seqs):
        if q.cam is not None:
            assert batch.set_depth_camera(s, q.cam) == 0, batch.last_error()
    assert batch.depth_camera(2) is None and batch.depth_camera(1).to_bytes() == seqs[1].cam.to_bytes()
    schedule, nxt = [], [0, 0, 0]
    for k in range(10):
        which = [nxt[0], None if k in (2, 3, 6) else nxt[1], nxt[2]]
        for s in range(3):
            if which[s] is not None:
                nxt[s] += 1
        schedule.append(which)
    got, inflight = [], 0
    for k, which in enumerate(schedule):
        fmt = hip_lib.DEPTH_U16 if k % 3 else hip_lib.DEPTH_F32
        g = [None if i is None else p.gray(i) for p, i in zip(P, which)]
        dd = [(None, p.depth(0, fmt)[1]) if i is None else p.depth(i, fmt) for p, i in zip(P, which)]
        assert batch.track_rgbd_device_async(g, [x[0] for x in dd], [q.H for q in seqs], [q.W for q in seqs], [p.gpitch for p in P], [x[1] for x in dd], fmt, SCALE) == 0, \
            batch.last_error()
        inflight += 1
        if inflight == 3:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    assert batch.last_error() == "", batch.last_error()
    check_against_own_oracles(oracle_lib, batch, [_BatchSeq(q) for q in seqs], schedule, got)
    batch.close()


def test_a_batch_with_more_depth_cameras_than_one_table_holds(hip_lib, oracle_lib):
    """25 RGB-D sequences with the half-size depth camera: each step takes a second k_depth_clear and a second k_depth_register launch, whose table holds
    sequence 24's descriptor alone.  Sequence s starts at frame s % 3; three steps, one at a time; sequences 0, 23 and 24 against oracle chains fed the
    numpy-registered planes (state, pose, all counters), every sequence TRACKING; each profile slot counts a step once.  (plane(0, 4) answers for sequence 0:
    the stage alone is held to numpy on sequence 24's last input instead.)"""
    need(hip_lib, *NEW)
    q, P = D.sequence("half"), planes("half")
    B, steps = 25, 3
    batch = hip_lib.LvtBatch(q.prm, B, 2)
    for s in range(B):
        assert batch.set_depth_camera(s, q.cam) == 0, batch.last_error()
    refs = []
    for o in range(3):
        orc, out = oracle_lib.Oracle(q.prm, 2), []
        for i in range(o, o + steps):
            Ro, to = orc.track_rgbd(q.gray[i], q.f32[i])
            out.append((np.array(Ro), np.array(to), orc.status, orc.counts()))
        assert [r[2] for r in out] == [2] * steps, "the oracle is not TRACKING on every frame"
        refs.append(out)
    batch.profile_enable(True)
    for k in range(steps):
        fr = [k + s % 3 for s in range(B)]
        dd = [P.depth(i, hip_lib.DEPTH_U16) for i in fr]
        assert batch.track_rgbd_device_async([P.gray(i) for i in fr], [x[0] for x in dd], q.H, q.W, P.gpitch, [x[1] for x in dd], hip_lib.DEPTH_U16, SCALE) == 0, \
            batch.last_error()
        R, t, st = batch.wait()
        assert batch.last_error() == "", batch.last_error()
        assert list(st) == [2] * B, (k, list(st))
        for s in (0, 23, 24):
            ref = refs[s % 3][k]
            e_t, e_R = pose_errors(R[s], t[s], ref[0], ref[1])
            print(f"sequence {s} step {k}: e_t {e_t:.2e} e_R {e_R:.2e}")
            assert e_t <= POSE_TOL and e_R <= POSE_TOL, f"sequence {s} step {k}: {e_t:.2e} {e_R:.2e}"
            ch = batch.counts(s)
            wrong = {n: (ch.get(n), v) for n, v in ref[3].items() if ch.get(n) != v}
            assert not wrong, f"sequence {s} step {k}: counters (hip, oracle) {wrong}"
    prof = dict(_profile_of(batch))
    assert prof["k_depth_clear"] == steps and prof["k_depth_register"] == steps, prof   # (a slot times a step's first launch)
    batch.close()
    check_stage(hip_lib, q.cam, q.prm, q.s_u16[steps - 1 + 24 % 3], SCALE)


def test_colour_handle_with_a_depth_camera(hip_lib, oracle_lib):
    """a colour (LVT_AMD_PIX_RGB8) handle with a depth camera: convert, register, track -- held to the oracle on the gray frames and the numpy planes"""
    q = D.sequence("half")
    sys_ = system_with_camera(hip_lib, q)
    assert sys_.set_pixel_format(hip_lib.PIX_RGB8) == 0, sys_.last_error()
    orc = oracle_lib.Oracle(q.prm, 2)
    for i in range(4):
        rgb = np.ascontiguousarray(np.repeat(q.gray[i][:, :, None], 3, axis=2))   # (R = G = B = g converts to g: 4899 + 9617 + 1868 = 2^14)
        R, t = sys_.track(rgb, q.s_u16[i], depth_scale=SCALE)
        Ro, to = orc.track_rgbd(q.gray[i], q.f32[i])
        held_to_oracle(sys_, orc, R, t, Ro, to, i)
        registered_plane_equals_numpy(sys_, q, i)
    sys_.close()


def _profile_of(h):
    return [(name, calls) for name, _ms, calls in h.profile_read()]


def test_launches(hip_lib):
    """with profiling on the two new names appear with calls == frames on a handle with a camera and not at all on one without; after set_depth_camera(None)
    the handle takes registered frames again and its records equal a fresh handle's"""
    need(hip_lib, *NEW)
    q, plain = D.sequence("same"), D.sequence("plain")
    new = ("k_depth_clear", "k_depth_register")
    ref = hip_lib.LvtSystem.create(plain.prm, 2)
    ref.profile_enable(True)
    fresh = []
    for i in range(4):
        R, t = ref.track(plain.gray[i], plain.f32[i])
        fresh.append(record(ref, R, t))
    rows = _profile_of(ref)
    assert rows and not [n for n, _ in rows if n in new], rows
    ref.close()

    sys_ = system_with_camera(hip_lib, q)
    sys_.profile_enable(True)
    for i in range(4):
        sys_.track(q.gray[i], q.s_u16[i], depth_scale=SCALE)
    prof = _profile_of(sys_)
    assert dict(prof)["k_depth_clear"] == 4 and dict(prof)["k_depth_register"] == 4, prof
    assert [(n, k) for n, k in prof if n not in new] == rows, (prof, rows)   # ... and nothing else changed
    sys_.close()

    sys_ = system_with_camera(hip_lib, q)
    assert sys_.depth_camera().to_bytes() == q.cam.to_bytes()
    assert sys_.set_depth_camera(None) == 0 and sys_.depth_camera() is None
    again = []
    for i in range(4):
        R, t = sys_.track(plain.gray[i], plain.f32[i])
        again.append(record(sys_, R, t))
    assert sys_.plane(0, 4).size == 0
    same_records(fresh, again, "a fresh handle / a handle whose camera was taken away")
    sys_.close()


def test_refusals_change_nothing(hip_lib, oracle_lib, tmp_path):
    """every refusal returns -1 with the reason in last_error(), and the next frame still tracks; get_depth_camera round-trips the record; a snapshot taken on a
    handle with a camera applies to one without, which continues"""
    import torch
    L = need(hip_lib, *NEW)
    q, plain = D.sequence("same"), D.sequence("plain")
    said = []

    def refused(h, rc, *words):
        assert rc == -1 and h.last_error() != "", (rc, h.last_error())
        for w in words:
            assert w in h.last_error(), (w, h.last_error())
        said.append(h.last_error())

    hip, orc = hip_lib.LvtSystem.create(plain.prm, 2), oracle_lib.Oracle(plain.prm, 2)
    nxt = [0]

    def next_frame():   # (registered frames: no camera has been accepted)
        i = nxt[0]; nxt[0] += 1
        Ro, to = orc.track_rgbd(plain.gray[i], plain.f32[i])
        R, t = hip.track(plain.gray[i], plain.f32[i])
        msgs = [m for m in diff_frame(hip, orc) if not (said and m == "hip error: " + said[-1])]
        assert not msgs, (i, msgs[:6])
        assert hip.depth_camera() is None and hip.plane(0, 4).size == 0

    def bad(**kw):
        c = copy.deepcopy(q.cam)
        c = D.make_camera(c.width, c.height, c.fx, c.fy, c.cx, c.cy, c.R, c.t)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    next_frame()
    for kw in (dict(width=0), dict(width=8193), dict(height=0), dict(height=8193)):
        refused(hip, hip.set_depth_camera(bad(**kw)), "8192")                        # a size outside 1 ... 8192
    next_frame()
    for kw in (dict(fx=float("nan")), dict(cy=float("inf")), dict(R=np.full((3, 3), np.nan)), dict(t=(0, -np.inf, 0))):
        refused(hip, hip.set_depth_camera(bad(**kw)), "non-finite")                  # a non-finite field
    for kw in (dict(fx=0.0), dict(fy=-1.0)):
        refused(hip, hip.set_depth_camera(bad(**kw)), "fx or fy")                    # fx or fy <= 0
    next_frame()
    refused(hip, L.lvt_amd_batch_set_depth_camera(hip._h, 0, C.byref(q.cam)), "not a batch")   # the batch call on a solo handle
    next_frame()
    P = planes("plain")
    ptr, pitch = P.depth(nxt[0], 0)
    assert hip.track_rgbd_device_async(P.gray(nxt[0]), ptr, plain.H, plain.W, P.gpitch, pitch, 0, SCALE) == 0
    refused(hip, hip.set_depth_camera(q.cam), "in flight")                           # a frame in flight
    R, t, st = hip.wait_status()
    orc.track_rgbd(plain.gray[nxt[0]], plain.f32[nxt[0]]); nxt[0] += 1
    assert st == orc.status == 2
    next_frame()
    # accepted now; per frame: a depth plane whose pitch does not hold a row of the camera's width
    wide = D.offset_camera(plain.prm, 400, 240)
    assert hip.set_depth_camera(wide) == 0, hip.last_error()
    assert hip.depth_camera().to_bytes() == wide.to_bytes()                          # the record round-trips
    before = hip.host_stats()["enqueued"]
    assert hip.track_rgbd_device(P.gray(0), ptr, plain.H, plain.W, P.gpitch, pitch, 0, SCALE) is None     # (a pitch of 332 elements)
    assert "pitch" in hip.last_error() and hip.host_stats()["enqueued"] == before
    said.append(hip.last_error())
    assert hip.set_depth_camera(None) == 0
    next_frame()
    hip.close()

    # handles that can never take a camera: refused, and they track their next stereo frames as the oracle does
    from parity_util import make_case
    wst, kp, _ = make_case("kitti", 0, 1.0, None, (320, 240))
    pairs = [wst.render_stereo(i) for i in range(2)]
    sorc = oracle_lib.Oracle(kp, 1)
    sref = [sorc.track(*p) for p in pairs]
    assert sorc.status == 2

    def tracks_stereo(h, what, full=False):
        for i, p in enumerate(pairs):
            R, t = h.track(*p)
            e_t, e_R = pose_errors(R, t, *sref[i])
            assert e_t <= POSE_TOL and e_R <= POSE_TOL, f"{what}, stereo frame {i}: {e_t:.2e} {e_R:.2e}"
        assert h.get_state() == 2, what
        if full:   # (the oracle stands behind frame 1: every stage of it)
            msgs = [m for m in diff_frame(h, sorc) if m != "hip error: " + said[-1]]
            assert not msgs, (what, msgs[:6])

    stereo = hip_lib.LvtSystem.create(kp, 1)
    refused(stereo, stereo.set_depth_camera(q.cam), "stereo")                        # a stereo handle
    assert stereo.depth_camera() is None
    tracks_stereo(stereo, "a stereo handle after the refusal", full=True)
    stereo.close()
    seat = hip_lib.LvtSystem.create(kp, 1, pooled=True)
    assert seat.ordering() == "pooled"
    refused(seat, seat.set_depth_camera(q.cam), "pooled")                            # a pooled seat
    kp.write_yaml(str(tmp_path / "cfg.yaml"))
    autos = [hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1) for _ in range(2)]
    assert autos[0].ordering() == "pooled"
    refused(autos[0], autos[0].set_depth_camera(q.cam))                              # an automatic seat
    for h, what in ((seat, "a pooled seat after the refusal"), (autos[0], "an automatic seat after the refusal")):
        assert h.depth_camera() is None
        tracks_stereo(h, what)
    for h in [seat] + autos:
        h.close()

    # a batch: the refusals change nothing -- its next step tracks registered frames in both sequences --, and once sequence 1 has a camera that sequence takes
    # the sensor's planes while sequence 0 stays on registered ones; each sequence against its own oracle
    batch = hip_lib.LvtBatch(plain.prm, 2, 2)
    for seq in (-1, 2):
        refused(batch, batch.set_depth_camera(seq, q.cam), "no sequence")             # seq out of range
        with pytest.raises(IndexError):
            batch.depth_camera(seq)
    refused(batch, L.lvt_amd_set_depth_camera(batch._h, C.byref(q.cam)), "per sequence")       # the solo call on a batch
    assert batch.depth_camera(0) is None and batch.depth_camera(1) is None
    Pq = planes("same")
    borc = [oracle_lib.Oracle(plain.prm, 2) for _ in range(2)]

    def batch_step(i, sensor1):
        fmt = hip_lib.DEPTH_U16 if sensor1 else hip_lib.DEPTH_F32   # (one format per call: sequence 0's registered plane is 16-bit beside a 16-bit sensor plane)
        d0, d1 = P.depth(i, fmt), (Pq if sensor1 else P).depth(i, fmt)
        assert batch.track_rgbd_device_async([P.gray(i)] * 2, [d0[0], d1[0]], plain.H, plain.W, P.gpitch, [d0[1], d1[1]], fmt, SCALE) == 0, batch.last_error()
        R, t, st = batch.wait()
        fed = [plain.f32[i], q.f32[i] if sensor1 else plain.f32[i]]
        for s_ in range(2):
            Ro, to = borc[s_].track_rgbd(plain.gray[i], fed[s_])
            e_t, e_R = pose_errors(R[s_], t[s_], Ro, to)
            assert st[s_] == borc[s_].status == 2 and e_t <= POSE_TOL and e_R <= POSE_TOL, f"batch sequence {s_} frame {i}: state {st[s_]}, {e_t:.2e} {e_R:.2e}"
            co, ch = borc[s_].counts(), batch.counts(s_)
            wrong = {k: (ch.get(k), v) for k, v in co.items() if ch.get(k) != v}
            assert not wrong, f"batch sequence {s_} frame {i}: counters (hip, oracle) {wrong}"

    batch_step(0, False)
    batch_step(1, False)
    assert batch.last_error() == said[-1], batch.last_error()   # (the last refusal's text stays; the steps added no report)
    assert batch.set_depth_camera(1, q.cam) == 0 and batch.depth_camera(0) is None and batch.depth_camera(1).to_bytes() == q.cam.to_bytes()
    batch_step(2, True)
    batch_step(3, True)
    batch.close()

    # not state: a snapshot taken on a handle with a camera applies to one without, and that handle continues on registered frames
    a = system_with_camera(hip_lib, q)
    orc = oracle_lib.Oracle(q.prm, 2)
    for i in range(5):
        a.track(q.gray[i], q.s_u16[i], depth_scale=SCALE)
        orc.track_rgbd(q.gray[i], q.f32[i])
    snap = a.snapshot()
    a.close()
    b = hip_lib.LvtSystem.create(q.prm, 2)
    assert b.restore(snap) == 0, b.last_error()
    assert b.depth_camera() is None
    for i in range(5, 8):
        R, t = b.track(q.gray[i], q.f32[i])            # (the numpy-registered planes: b has no camera)
        Ro, to = orc.track_rgbd(q.gray[i], q.f32[i])
        held_to_oracle(b, orc, R, t, Ro, to, i)
    b.close()
    torch.cuda.synchronize()
