"""DEPTH GUARD on the GPU: lvt_amd_set_depth_guard / lvt_amd_batch_set_depth_guard, the launch k_depth_guard directly behind the gather step,
lvt_amd_get_depth_guard / _stats and the stage entry lvt_amd_depth_guard_features.  No expected value comes from this library: the rule is restated in numpy
(depth_guard_util, held to hand-written planes and a scalar walk by test_depth_guard.py) and the tracker is held to the UNCHANGED oracle through one
equivalence -- detected corners are integers, so a guarded frame equals Oracle.track_rgbd(gray, guarded_depth(depth)), the complete diff_frame.
Every oracle is asserted TRACKING before anything is compared, and every guarded comparison asserts that its record drops at least one feature of the frame.
Frames in flight together are held by state and pose, frame by frame, and by the complete diff behind the last one.  The world: tum 0 at 322 x 242, 8 frames.
(lvt_track_with_external_corners is a stereo entry and a stereo handle has no guard: fractional positions reach the rule through the stage entry only.)"""
import ctypes as C

import numpy as np
import pytest

import depth_guard_util as DG
import mask_util as MU
from parity_util import make_case, diff_frame, pose_errors, POSE_TOL
from rgbd_util import RSeq, SCALE, quantise, check_against_own_oracles

pytestmark = pytest.mark.gpu

N = 8
OTHER = DG.Guard(2, 24, 0.01, 0.02)      # a second record: all but one of the 5 x 5 window (62 - 70 features of a frame)
f32 = np.float32


def record_of(hip_lib, g):
    return hip_lib.DepthGuard(g.radius, g.min_support, g.tol_abs, g.tol_rel)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
class World:
    """gray frames, the rendered fp32 depth `f32`, its 16-bit quantisation `u16` and that one's conversion `q32`; guarded planes are made once per record"""

    def __init__(self, overrides=None, size=(322, 242)):
        self.world, self.prm, sensor = make_case("tum", 0, 1.0, overrides, size)
        assert sensor == 2
        self.W, self.H = self.world.W, self.world.H
        self.near, self.far = self.prm.near_plane_distance, self.prm.far_plane_distance
        fr = [self.world.render_rgbd(i) for i in range(N)]
        self.gray = [np.ascontiguousarray(g) for g, _ in fr]
        self.f32 = [np.ascontiguousarray(d, dtype=f32) for _, d in fr]
        self.u16 = [quantise(d) for d in self.f32]
        self.q32 = [u.astype(f32) * SCALE for u in self.u16]
        self._guarded, self._corners, self._dev = {}, {}, None

    def corners(self, i):
        from oracle import pyoracle as O
        if i not in self._corners:
            self._corners[i] = O.detect_grid(self.gray[i], self.prm)[0]
        return self._corners[i]

    def guarded(self, i, cfg, kind="f32", planes=None):
        """the plane the oracle is fed for frame i under cfg; asserts that the guard drops a feature of the frame"""
        key = (i, cfg, kind)
        if key not in self._guarded:
            d = (planes or getattr(self, kind))[i]
            n, _ = DG.dropped_share(self.corners(i), d, cfg, self.near, self.far, f"frame {i}")
            feats = DG.features_of(self.corners(i), d, self.near, self.far, self.W, self.H)
            self._guarded[key] = (DG.guarded_depth(d, cfg, self.near, self.far), len(feats) - n, n)
        return self._guarded[key]

    def device(self):
        if self._dev is None:
            self._dev = RSeq.from_frames(self.prm, self.gray, self.q32, self.u16)
        return self._dev


_ONCE = {}


def world(barrel=False):
    key = "barrel" if barrel else "w"
    if key not in _ONCE:
        _ONCE[key] = World({"k1": -0.25} if barrel else None)
    return _ONCE[key]


def guarded_system(hip_lib, q, cfg):
    hip = hip_lib.LvtSystem.create(q.prm, 2)
    assert hip.set_depth_guard(record_of(hip_lib, cfg)) == 0, hip.last_error()
    return hip


def hold(hip, orc, R, t, Ro, to, i):
    assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
    msgs = diff_frame(hip, orc)
    assert not msgs, (i, msgs[:6])
    e_t, e_R = pose_errors(np.asarray(R), np.asarray(t), np.asarray(Ro), np.asarray(to))
    assert e_t <= POSE_TOL and e_R <= POSE_TOL, f"frame {i}: e_t {e_t:.2e} e_R {e_R:.2e}"


def run_async(hip, orc, submit, oracle_plane, q, depth=3):
    """n frames, `depth` in flight: state and pose of each as it is collected, the complete diff once the handle is drained"""
    inflight = []

    def collect():
        i = inflight.pop(0)
        R, t, st = hip.wait_status()
        Ro, to = orc.track_rgbd(q.gray[i], oracle_plane(i))
        e_t, e_R = pose_errors(R, t, np.asarray(Ro), np.asarray(to))
        assert st == orc.status == 2 and e_t <= POSE_TOL and e_R <= POSE_TOL, f"frame {i}: state {st} / {orc.status}, {e_t:.2e} {e_R:.2e}"
        if not inflight:
            msgs = diff_frame(hip, orc)
            assert not msgs, f"frame {i}: {msgs[:6]}"
    for i in range(N):
        assert submit(i) == 0, hip.last_error()
        inflight.append(i)
        if len(inflight) == depth:
            collect()
    while inflight:
        collect()
    assert hip.last_error() == "", hip.last_error()


# ---- 1. the stage entry against numpy, bit for bit --------------------------------------------------------------------------------------------
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4096]
NEAR, FAR = 0.1, 5.0


def stage_plane(W, H, pad, u16, rng):
    """a plane of 4 x 4 blocks at five levels with noise about as large as the tolerance, one pixel in ten a special value: NaN, both infinities, both zeros,
    the near and the far plane and their fp32 neighbours (16-bit: 0, 65535 and the raws around near / scale and far / scale).  A view into rows of W + pad
    elements whose padding holds a valid depth of 2 m: a wrong pitch, or a window that is not clipped at the plane's edge, would find support there"""
    by, bx = np.mgrid[0:H, 0:W]
    level = np.array([1.0, 1.04, 1.5, 3.0, 4.9], f32)[rng.integers(0, 5, ((H + 3) // 4, (W + 3) // 4))][by // 4, bx // 4]
    plane = (level + rng.uniform(-0.03, 0.03, (H, W)).astype(f32)).astype(f32)
    special = rng.random((H, W)) < 0.1
    if u16:
        store = np.full((H, W + pad), 10000, np.uint16)
        raw = np.clip(np.rint(plane.astype(np.float64) * 5000.0), 0, 65535).astype(np.uint16)
        raw[special] = rng.choice(np.array([0, 65535, 499, 500, 501, 24999, 25000, 25001], np.uint16), size=int(special.sum()))
        store[:, :W] = raw
    else:
        store = np.full((H, W + pad), 2.0, f32)
        n, fa = f32(NEAR), f32(FAR)
        plane[special] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, n, np.nextafter(n, f32(0)), np.nextafter(n, f32(1)), fa, np.nextafter(fa, f32(0)),
                                              np.nextafter(fa, f32(9))], f32), size=int(special.sum()))
        store[:, :W] = plane
    return store[:, :W]


def stage_features(W, H, n, rng):
    """positions: seven in ten inside the plane with any fraction, one in ten on a pixel exactly, one in ten around and beyond the plane's edges (and NaN,
    infinities), one in ten any bit pattern; every other array any bit pattern"""
    def bits(k):
        return rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32).view(f32)
    pos = []
    for size in (W, H):
        p = rng.uniform(0, size, n).astype(f32)
        kind = rng.random(n)
        whole = kind < 0.1
        p[whole] = np.trunc(p[whole])
        edge = (kind >= 0.1) & (kind < 0.2)
        p[edge] = rng.choice(np.array([-1.0, np.nextafter(f32(-1), f32(0)), -0.5, -0.0, size - 0.5, np.nextafter(f32(size), f32(0)), size, size + 3, -7.25, 1e9, -1e9,
                                       3e38, np.inf, -np.inf, np.nan], f32), size=int(edge.sum()))
        anyb = (kind >= 0.2) & (kind < 0.3)
        p[anyb] = bits(int(anyb.sum()))
        pos.append(p)
    i16 = [rng.integers(-32768, 32768, n).astype(np.int16) for _ in range(2)]
    return [bits(n), bits(n), bits(n), pos[0], pos[1], bits(n), i16[0], i16[1]]


@pytest.mark.parametrize("u16", [False, True], ids=["fp32", "u16"])
@pytest.mark.parametrize("W,H,pad", [(7, 5, 3), (64, 48, 1), (321, 243, 7)], ids=["7x5", "64x48", "321x243"])
def test_stage_entry_equals_numpy_bit_for_bit(hip_lib, W, H, pad, u16):
    rng = np.random.default_rng(100 * W + (1 if u16 else 0))
    plane = stage_plane(W, H, pad, u16, rng)
    assert plane.strides[0] == (W + pad) * plane.itemsize
    scale = SCALE if u16 else None
    full = stage_features(W, H, 4096, rng)
    dropped_some = kept_some = False
    for radius in (1, 2, 3):
        most = (2 * radius + 1) ** 2 - 1
        for min_support in (1, most // 2, most):
            cfg = DG.Guard(radius, min_support, 0.01, 0.02)
            keep_all = DG.keep_features(full[3], full[4], plane, cfg, NEAR, FAR, scale)
            for n in SIZES:
                arrays, keep = [a[:n] for a in full], keep_all[:n]
                got = hip_lib.depth_guard_features(*arrays, plane, record_of(hip_lib, cfg), NEAR, FAR, depth_scale=float(SCALE) if u16 else 0.0)
                k = int(keep.sum())
                assert got[0] == k, (cfg, n, got[0], k)
                for name, a, g in zip(("x", "y", "resp", "bx", "by", "depth", "hcx", "hcy"), arrays, got[1:]):
                    bits = np.uint32 if a.dtype == np.float32 else np.int16
                    assert np.array_equal(g[:k].view(bits), a[keep].view(bits)), (cfg, n, name, "kept")
                    assert np.array_equal(g[k:].view(bits), a[k:].view(bits)), (cfg, n, name, "the tail was written")
            kept_some |= bool(keep_all.any())
            dropped_some |= bool((~keep_all).any())
            if min_support == most // 2 and W > 7:
                assert 0.05 < keep_all.mean() < 0.95, (cfg, keep_all.mean())
    assert dropped_some and kept_some


def test_stage_entry_refusals(hip_lib):
    rng = np.random.default_rng(1)
    plane = np.ascontiguousarray(stage_plane(64, 48, 0, False, rng))
    arrays = stage_features(64, 48, 10, rng)
    L = hip_lib.load_library()
    p = [a.ctypes.data_as(C.c_void_p) for a in arrays]
    d = plane.ctypes.data_as(C.c_void_p)
    ok, flo = hip_lib.DepthGuard(1, 4, 0.01, 0.02), C.c_float

    def args(n=10, ptrs=p, depth=d, fmt=0, scale=0.0, w=64, h=48, pitch=64, cfg=ok):
        return (n, *ptrs, depth, fmt, flo(scale), w, h, pitch, flo(NEAR), flo(FAR), C.byref(cfg) if cfg is not None else None)
    bad = [args(n=4097), args(n=-1), args(pitch=63), args(depth=None), args(w=0), args(ptrs=p[:4] + [None] + p[5:]), args(cfg=None), args(fmt=2),
           args(fmt=1, scale=0.0), args(fmt=1, scale=float("nan")), args(cfg=hip_lib.DepthGuard(0, 1, 0.01, 0.02)), args(cfg=hip_lib.DepthGuard(4, 1, 0.01, 0.02)),
           args(cfg=hip_lib.DepthGuard(1, 0, 0.01, 0.02)), args(cfg=hip_lib.DepthGuard(1, 9, 0.01, 0.02)), args(cfg=hip_lib.DepthGuard(2, 25, 0.01, 0.02)),
           args(cfg=hip_lib.DepthGuard(1, 4, -0.01, 0.02)), args(cfg=hip_lib.DepthGuard(1, 4, 0.01, float("inf"))), args(cfg=hip_lib.DepthGuard(1, 4, float("nan"), 0.0))]
    for a in bad:
        assert L.lvt_amd_depth_guard_features(*a) == -1
        err = L.lvt_amd_last_error(None).decode()
        assert err.startswith("lvt_amd_depth_guard_features: ") and err.endswith("(nothing was changed)"), err
    for cfg in (hip_lib.DepthGuard(1, 8, 0.0, 0.0), hip_lib.DepthGuard(2, 24, 0.01, 0.02), hip_lib.DepthGuard(3, 48, 0.01, 0.02)):   # the ranges' ends
        assert L.lvt_amd_depth_guard_features(*args(cfg=cfg)) >= 0, L.lvt_amd_last_error(None)
    g = hip_lib.depth_guard_default()
    assert (g.radius, g.min_support, f32(g.tol_abs), f32(g.tol_rel)) == (1, 4, f32(0.01), f32(0.02))


# ---- 2. sequences held to the oracle -------------------------------------------------------------------------------------------------------------
def test_guarded_frames_through_track_rgbd(hip_lib, oracle_lib):
    """lvt_amd_track_rgbd under {1, 6, 0.01, 0.02}: the complete diff on every frame, the statistics numpy's, and an unguarded handle on the same frames has
    more features on every frame (what this file fails on without the feature)"""
    q = world()
    hip, plain, orc = guarded_system(hip_lib, q, DG.STRICT), hip_lib.LvtSystem.create(q.prm, 2), oracle_lib.Oracle(q.prm, 2)
    assert hip.depth_guard_stats() is None, "statistics before the first guarded frame"
    assert plain.depth_guard() is None and plain.depth_guard_stats() is None
    for i in range(N):
        plane, kept, dropped = q.guarded(i, DG.STRICT)
        Ro, to = orc.track_rgbd(q.gray[i], plane)
        R, t = hip.track(q.gray[i], q.f32[i])
        hold(hip, orc, R, t, Ro, to, i)
        assert hip.depth_guard_stats() == {"kept": kept, "dropped": dropped}, (i, hip.depth_guard_stats(), kept, dropped)
        plain.track(q.gray[i], q.f32[i])
        assert plain.counts()["n_left"] == kept + dropped > hip.counts()["n_left"] == kept, i
        assert dropped >= 0.10 * len(q.corners(i)), (i, dropped, len(q.corners(i)))
    assert hip.last_error() == "", hip.last_error()
    g = hip.depth_guard()
    assert (g.radius, g.min_support, f32(g.tol_abs), f32(g.tol_rel)) == (1, 6, f32(0.01), f32(0.02))


def test_guarded_frames_through_track_rgbd_async(hip_lib, oracle_lib):
    """lvt_amd_track_rgbd_async on host frames, three in flight"""
    q = world()
    hip, orc = guarded_system(hip_lib, q, DG.STRICT), oracle_lib.Oracle(q.prm, 2)
    run_async(hip, orc, lambda i: hip.track_async(q.gray[i], q.f32[i]), lambda i: q.guarded(i, DG.STRICT)[0], q)
    assert hip.depth_guard_stats() == {"kept": q.guarded(N - 1, DG.STRICT)[1], "dropped": q.guarded(N - 1, DG.STRICT)[2]}


def test_guarded_device_planes_at_an_odd_pitch(hip_lib, oracle_lib):
    """lvt_amd_track_rgbd_device_async, three in flight: fp32 planes in HBM with rows of W + 12 elements (whose padding holds a valid 3 m) on even frames, 16-bit
    planes at a 2-byte-but-not-4-byte aligned address with rows of W + 6 elements (padding 15000 = 3 m) on odd frames"""
    q = world()
    dev = q.device()
    hip, orc = guarded_system(hip_lib, q, DG.STRICT), oracle_lib.Oracle(q.prm, 2)
    assert dev.f32_pitch() == 4 * (q.W + 12) and dev.u16_pitch() == 2 * (q.W + 6)

    def submit(i):
        if i % 2:
            return hip.track_rgbd_device_async(dev.gray_ptr(i), dev.u16_ptr(i), q.H, q.W, dev.gpitch, dev.u16_pitch(), hip_lib.DEPTH_U16, SCALE)
        return hip.track_rgbd_device_async(dev.gray_ptr(i), dev.f32_ptr(i), q.H, q.W, dev.gpitch, dev.f32_pitch(), hip_lib.DEPTH_F32, 1.0)
    run_async(hip, orc, submit, lambda i: q.guarded(i, DG.STRICT, "q32")[0], q)


def test_guarded_16_bit_frames(hip_lib, oracle_lib):
    """lvt_amd_track_rgbd16 with LVT_AMD_DEPTH_U16: the guard reads the raws and converts them as the gather step does; the oracle is fed the guarded conversion"""
    q = world()
    hip, orc = guarded_system(hip_lib, q, DG.STRICT), oracle_lib.Oracle(q.prm, 2)
    for i in range(N):
        plane, kept, dropped = q.guarded(i, DG.STRICT, "q32")
        assert np.array_equal(plane != 0, DG.guarded_depth(q.u16[i], DG.STRICT, q.near, q.far, SCALE) != 0)
        Ro, to = orc.track_rgbd(q.gray[i], plane)
        R, t = hip.track(q.gray[i], q.u16[i], depth_scale=SCALE)
        hold(hip, orc, R, t, Ro, to, i)
        assert hip.depth_guard_stats() == {"kept": kept, "dropped": dropped}, i


def test_a_depth_camera_and_a_guard(hip_lib, oracle_lib):
    """unregistered 16-bit depth from a camera 5 cm to the side: the guard reads the REGISTERED plane (plane 4), whose holes (+inf) are not valid; the oracle
    is fed the guarded numpy-registered plane"""
    import depth_reg_util as D
    q = world()
    if "cam" not in _ONCE:
        _ONCE["cam"] = D.DSeq(0, (322, 242), N, lambda p: D.offset_camera(p, 322, 242))
    c = _ONCE["cam"]
    assert min(c.holes) > 0.005, "the registered planes have no holes"
    assert all(np.array_equal(a, b) for a, b in zip(c.gray, q.gray)), "the two sequences are one world"
    hip, orc = guarded_system(hip_lib, q, DG.STRICT), oracle_lib.Oracle(c.prm, 2)
    assert hip.set_depth_camera(c.cam) == 0, hip.last_error()
    for i in range(N):
        plane, kept, dropped = q.guarded(i, DG.STRICT, "registered", planes=c.f32)
        Ro, to = orc.track_rgbd(c.gray[i], plane)
        R, t = hip.track(c.gray[i], c.s_u16[i], depth_scale=SCALE)
        hold(hip, orc, R, t, Ro, to, i)
        assert hip.depth_guard_stats() == {"kept": kept, "dropped": dropped}, i


def test_a_mask_and_a_guard(hip_lib, oracle_lib):
    """the guard first, then the mask: the mask's statistics count what the guard left"""
    q = world()
    m = MU.bonnet(q.W, q.H)
    hip, orc = guarded_system(hip_lib, q, DG.STRICT), oracle_lib.Oracle(q.prm, 2)
    assert hip.set_mask(m, None) == 0, hip.last_error()
    for i in range(N):
        plane, kept, dropped = q.guarded(i, DG.STRICT)
        Ro, to = orc.track_rgbd(q.gray[i], MU.masked_depth(plane, m))
        R, t = hip.track(q.gray[i], q.f32[i])
        hold(hip, orc, R, t, Ro, to, i)
        feats = DG.features_of(q.corners(i), q.f32[i], q.near, q.far, q.W, q.H)
        left = feats[DG.keep_features(feats[:, 0], feats[:, 1], q.f32[i], DG.STRICT, q.near, q.far)]
        mk = MU.keep_rule(left[:, 0], left[:, 1], m)
        assert hip.depth_guard_stats() == {"kept": kept, "dropped": dropped} and len(left) == kept, i
        assert hip.mask_stats() == {"kept": (int(mk.sum()), 0), "dropped": (int((~mk).sum()), 0)} and 0 < mk.sum() < kept, (i, hip.mask_stats())
        assert hip.counts()["n_left"] == int(mk.sum())


def test_a_guard_behind_a_barrel_lens(hip_lib, oracle_lib):
    """k1 = -0.25: the features are reported at undistorted coordinates, the guard reads the raw pixel the gather step read"""
    q = world(barrel=True)
    assert q.prm.k1 < 0
    hip, orc = guarded_system(hip_lib, q, DG.STRICT), oracle_lib.Oracle(q.prm, 2)
    for i in range(N):
        plane, kept, dropped = q.guarded(i, DG.STRICT)
        Ro, to = orc.track_rgbd(q.gray[i], plane)
        R, t = hip.track(q.gray[i], q.f32[i])
        hold(hip, orc, R, t, Ro, to, i)
        xy = hip.features(0)[0]
        assert np.any(xy != np.rint(xy)) and hip.depth_guard_stats() == {"kept": kept, "dropped": dropped}, i


class _Fed:
    """what rgbd_util.check_against_own_oracles reads of a sequence: the planes its ORACLE is fed"""

    def __init__(self, prm, gray, planes):
        self.prm, self.gray, self.f32 = prm, gray, planes


def test_mixed_batch_of_guarded_plain_and_absent(hip_lib, oracle_lib):
    """four RGB-D sequences in one chain, three steps in flight, the depth format changing between steps: 0 = 322 x 242 under {1, 6}; 1 = 322 x 242 under
    {2, 24}; 2 = 320 x 240, no guard; 3 = 322 x 242 under the default record, sitting out steps 2 and 4.  Each is held to its own oracle on its own planes"""
    import depth_reg_util as D
    q = world()
    small = D.sequence("plain")
    sm = _ONCE.setdefault("small", RSeq.from_frames(small.prm, small.gray[:N], small.f32[:N], small.s_u16[:N]))
    dev = q.device()
    seqs, cfgs = [dev, dev, sm, dev], [DG.STRICT, OTHER, None, DG.DEFAULT]
    batch = hip_lib.LvtBatch.create_mixed([s.prm for s in seqs], 2)
    for s, cfg in enumerate(cfgs):
        if cfg is not None:
            assert batch.set_depth_guard(s, record_of(hip_lib, cfg)) == 0, batch.last_error()
    assert batch.depth_guard(2) is None and batch.depth_guard(1).min_support == 24 and batch.depth_guard_stats(0) is None
    schedule, nxt = [], [0, 0, 0, 0]
    for k in range(N):
        which = [nxt[0], nxt[1], nxt[2], None if k in (2, 4) else nxt[3]]
        for s in range(4):
            nxt[s] += which[s] is not None
        schedule.append(which)
    got, inflight = [], 0
    for k, which in enumerate(schedule):
        u16 = k % 2 == 1
        g = [None if i is None else s.gray_ptr(i) for s, i in zip(seqs, which)]
        d = [None if i is None else (s.u16_ptr(i) if u16 else s.f32_ptr(i)) for s, i in zip(seqs, which)]
        dp = [s.u16_pitch() if u16 else s.f32_pitch() for s in seqs]
        rc = batch.track_rgbd_device_async(g, d, [s.H for s in seqs], [s.W for s in seqs], [s.gpitch for s in seqs], dp, hip_lib.DEPTH_U16 if u16 else hip_lib.DEPTH_F32, SCALE)
        assert rc == 0, batch.last_error()
        inflight += 1
        if inflight == 3:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    assert batch.last_error() == "", batch.last_error()
    fed = [_Fed(s.prm, s.gray, s.f32 if cfg is None else [q.guarded(i, cfg, "q32")[0] for i in range(N)]) for s, cfg in zip(seqs, cfgs)]
    check_against_own_oracles(oracle_lib, batch, fed, schedule, got)
    for s, cfg in enumerate(cfgs):
        last = schedule[-1][s]
        want = None if cfg is None else {"kept": q.guarded(last, cfg, "q32")[1], "dropped": q.guarded(last, cfg, "q32")[2]}
        assert batch.depth_guard_stats(s) == want, (s, batch.depth_guard_stats(s), want)
    batch.close()


def test_a_batch_with_more_sequences_than_one_table_holds(hip_lib, oracle_lib):
    """34 RGB-D sequences, one table holds 32, so slot k of the second launch is sequence 32 + k: sequence 0 under {1, 6} and sequence 1 under {2, 24} are the
    records a slot of the second table must NOT inherit; sequence 32 has no guard; sequence 33 runs under the default record and sits steps 1 and 3 out;
    the others have no guard.  Four steps, three in flight, every sequence held to its own oracle on its own planes; a sequence without a guard, and one that
    sat the last step out, have no statistics"""
    q = world()
    dev = q.device()
    B = 34
    cfgs = [DG.STRICT, OTHER] + [None] * 30 + [None, DG.DEFAULT]
    batch = hip_lib.LvtBatch.create_mixed([q.prm] * B, 2)
    for s, cfg in enumerate(cfgs):
        if cfg is not None:
            assert batch.set_depth_guard(s, record_of(hip_lib, cfg)) == 0, batch.last_error()
    schedule, nxt = [], [0] * B
    for k in range(4):
        which = [None if (s == 33 and k in (1, 3)) else nxt[s] for s in range(B)]
        for s in range(B):
            nxt[s] += which[s] is not None
        schedule.append(which)
    got, inflight = [], 0
    for k, which in enumerate(schedule):
        u16 = k % 2 == 1
        g = [None if i is None else dev.gray_ptr(i) for i in which]
        d = [None if i is None else (dev.u16_ptr(i) if u16 else dev.f32_ptr(i)) for i in which]
        rc = batch.track_rgbd_device_async(g, d, [q.H] * B, [q.W] * B, [dev.gpitch] * B, [dev.u16_pitch() if u16 else dev.f32_pitch()] * B,
                                           hip_lib.DEPTH_U16 if u16 else hip_lib.DEPTH_F32, SCALE)
        assert rc == 0, batch.last_error()
        inflight += 1
        if inflight == 3:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    assert batch.last_error() == "", batch.last_error()
    planes = {cfg: (dev.f32 if cfg is None else [q.guarded(i, cfg, "q32")[0] for i in range(4)]) for cfg in set(cfgs)}
    check_against_own_oracles(oracle_lib, batch, [_Fed(q.prm, q.gray, planes[cfg]) for cfg in cfgs], schedule, got)
    for s, cfg in enumerate(cfgs):
        want = None if (cfg is None or s == 33) else {"kept": q.guarded(3, cfg, "q32")[1], "dropped": q.guarded(3, cfg, "q32")[2]}
        assert batch.depth_guard_stats(s) == want, (s, batch.depth_guard_stats(s), want)
    plain = q.guarded(3, DG.STRICT, "q32")
    assert batch.counts(32)["n_left"] == plain[1] + plain[2] > batch.counts(0)["n_left"] == plain[1], "sequence 32 was filtered"
    batch.close()


# ---- 3. the property's behaviour ---------------------------------------------------------------------------------------------------------------
def test_set_unset_and_set_again_between_frames(hip_lib, oracle_lib):
    """frames 0 - 2 under {1, 6}, 3 - 4 without a guard -- the unguarded oracle --, 5 - 7 under {2, 24}: ONE oracle chain"""
    q = world()
    hip, orc = guarded_system(hip_lib, q, DG.STRICT), oracle_lib.Oracle(q.prm, 2)
    plan = [DG.STRICT] * 3 + [None] * 2 + [OTHER] * 3
    for i in range(N):
        if i in (3, 5):
            assert hip.set_depth_guard(record_of(hip_lib, plan[i]) if plan[i] else None) == 0, hip.last_error()
            assert hip.depth_guard_stats() is None, "the last frame went in under another record"
            assert (hip.depth_guard() is None) == (plan[i] is None)
        if i == 4:
            assert hip.set_depth_guard(None) == 0, "unsetting what is not set"
        Ro, to = orc.track_rgbd(q.gray[i], q.guarded(i, plan[i])[0] if plan[i] else q.f32[i])
        R, t = hip.track(q.gray[i], q.f32[i])
        hold(hip, orc, R, t, Ro, to, i)
        st = hip.depth_guard_stats()
        assert (st is None) if plan[i] is None else (st == {"kept": q.guarded(i, plan[i])[1], "dropped": q.guarded(i, plan[i])[2]}), (i, st)
    hip.reset()   # (a property, not state: the record stays)
    assert hip.depth_guard().min_support == 24
    R, t = hip.track(q.gray[0], q.f32[0])
    assert hip.depth_guard_stats() == {"kept": q.guarded(0, OTHER)[1], "dropped": q.guarded(0, OTHER)[2]}


def test_a_guard_that_drops_nothing_changes_no_bit_and_no_snapshot_byte(hip_lib, oracle_lib):
    """{1, 1, 100, 100}: every valid neighbour supports, and the synthetic plane has no invalid pixel: the guarded handle's poses and features are the plain
    handle's bit for bit, and so are its snapshot's bytes -- a snapshot does not know the guard"""
    q = world()
    hip, plain = guarded_system(hip_lib, q, DG.Guard(1, 1, 100.0, 100.0)), hip_lib.LvtSystem.create(q.prm, 2)
    for i in range(4):
        Ra, ta = hip.track(q.gray[i], q.f32[i])
        Rb, tb = plain.track(q.gray[i], q.f32[i])
        assert np.array_equal(Ra, Rb) and np.array_equal(ta, tb), f"frame {i}"
        for a, b in zip(hip.features(0), plain.features(0)):
            assert np.array_equal(a, b), f"frame {i}"
        assert hip.depth_guard_stats() == {"kept": plain.counts()["n_left"], "dropped": 0}
    assert hip.get_state() == plain.get_state() == 2
    assert hip.snapshot().to_bytes() == plain.snapshot().to_bytes(), "the snapshot of a guarded handle knows its guard"


def _profile_of(h):
    return [(name, calls) for name, _ms, calls in h.profile_read()]


def test_launch_accounting(hip_lib, oracle_lib):
    """a handle that never set a guard has no k_depth_guard row; a guarded handle reports exactly one call per frame and every other row as the plain one"""
    q = world()
    plain = hip_lib.LvtSystem.create(q.prm, 2)
    plain.profile_enable(True)
    for i in range(4):
        plain.track(q.gray[i], q.f32[i])
    rows = _profile_of(plain)
    assert rows and not [n for n, _ in rows if "guard" in n], rows
    assert dict(rows)["k_score"] == 4
    plain.close()   # (a handle created beside a live one orders its streams with events: other rows)
    hip = guarded_system(hip_lib, q, DG.STRICT)
    hip.profile_enable(True)
    for i in range(4):
        hip.track(q.gray[i], q.f32[i])
    prof = _profile_of(hip)
    assert dict(prof)["k_depth_guard"] == 4, prof
    assert [(n, k) for n, k in prof if n != "k_depth_guard"] == rows, (prof, rows)
    assert hip.set_depth_guard(None) == 0
    hip.track(q.gray[4], q.f32[4])
    assert dict(_profile_of(hip))["k_depth_guard"] == 4, "an unset guard still launches"


# ---- 4. every refusal, in the contract's order ---------------------------------------------------------------------------------------------------
U = " (nothing was changed)"
WHO = "lvt_amd_set_depth_guard: "
TEXT = {
    "pooled": WHO + "a pooled handle (pooled handles are stereo only)" + U,
    "stereo": WHO + "a stereo handle (it has no depth plane to guard)" + U,
    "solo call on a batch": WHO + "a batch handle takes its depth guards per sequence through lvt_amd_batch_set_depth_guard" + U,
    "batch call on a solo": WHO + "lvt_amd_batch_set_depth_guard on a handle that is not a batch (use lvt_amd_set_depth_guard)" + U,
    "seq 2": WHO + "no sequence 2 in this handle" + U,
    "seq -1": WHO + "no sequence -1 in this handle" + U,
    "radius 0": WHO + "a depth guard with radius = 0 (1 ... 3)" + U,
    "radius 4": WHO + "a depth guard with radius = 4 (1 ... 3)" + U,
    "support 0": WHO + "a depth guard with min_support = 0 at radius 1 (1 ... 8)" + U,
    "support 25": WHO + "a depth guard with min_support = 25 at radius 2 (1 ... 24)" + U,
    "tol_abs": WHO + "a depth guard whose tol_abs is not finite and >= 0" + U,
    "tol_rel": WHO + "a depth guard whose tol_rel is not finite and >= 0" + U,
    "in flight": WHO + "frames in flight: set the depth guard before the first frame or after every frame has been collected" + U,
}


def test_every_refusal_says_its_sentence_and_changes_nothing(hip_lib, oracle_lib, tmp_path):
    """each refusal returns -1 and leaves its complete sentence; where two objections apply the earlier one of the contract's order is named -- the handle's
    kind, the sensor, the spelling, the sequence, the record, frames in flight --; and the guarded handle keeps its record and goes on tracking, every frame
    against the oracle under the record it had"""
    q = world()
    L, DGd = hip_lib.load_library(), hip_lib.DepthGuard
    ok, seen = DGd(2, 24, 0.01, 0.02), []
    bad = {"radius 0": DGd(0, 1, 0.01, 0.02), "radius 4": DGd(4, 1, 0.01, 0.02), "support 0": DGd(1, 0, 0.01, 0.02), "support 25": DGd(2, 25, 0.01, 0.02),
           "tol_abs": DGd(1, 4, -1.0, 0.02), "tol_rel": DGd(1, 4, 0.01, float("nan"))}

    def refused(h, rc, key):
        assert rc == -1 and h.last_error() == TEXT[key], (key, rc, h.last_error())
        seen.append(key)

    assert L.lvt_amd_set_depth_guard(None, C.byref(ok)) == -1 and L.lvt_amd_batch_set_depth_guard(None, 0, C.byref(ok)) == -1     # a bad handle: no report
    assert L.lvt_amd_get_depth_guard(None, 0, None) == -1 and L.lvt_amd_get_depth_guard_stats(None, 0, None) == -1
    hip, orc, i = guarded_system(hip_lib, q, DG.STRICT), oracle_lib.Oracle(q.prm, 2), 0

    def next_frame():
        nonlocal i
        plane, kept, dropped = q.guarded(i, DG.STRICT)
        Ro, to = orc.track_rgbd(q.gray[i], plane)
        R, t = hip.track(q.gray[i], q.f32[i])
        assert orc.status == 2
        msgs = [x for x in diff_frame(hip, orc) if not x.startswith("hip error: ")]
        assert not msgs, (i, msgs[:6])
        assert hip.depth_guard().min_support == 6 and hip.depth_guard_stats() == {"kept": kept, "dropped": dropped}
        i += 1

    next_frame()
    refused(hip, L.lvt_amd_batch_set_depth_guard(hip._h, 0, C.byref(ok)), "batch call on a solo")
    refused(hip, L.lvt_amd_batch_set_depth_guard(hip._h, 5, C.byref(bad["radius 0"])), "batch call on a solo")      # the spelling before the sequence and the record
    next_frame()
    for key, rec in bad.items():
        refused(hip, hip.set_depth_guard(rec), key)
    next_frame()
    dev = q.device()
    for call, key in ((lambda: hip.set_depth_guard(ok), "in flight"), (lambda: hip.set_depth_guard(None), "in flight"),
                      (lambda: hip.set_depth_guard(bad["tol_abs"]), "tol_abs")):                                        # the record before the frames in flight
        assert hip.track_rgbd_device_async(dev.gray_ptr(i), dev.f32_ptr(i), q.H, q.W, dev.gpitch, dev.f32_pitch(), hip_lib.DEPTH_F32, 1.0) == 0, hip.last_error()
        refused(hip, call(), key)
        Ro, to = orc.track_rgbd(q.gray[i], q.guarded(i, DG.STRICT, "q32")[0])
        R, t, st = hip.wait_status()
        assert st == orc.status == 2
        i += 1
    next_frame()
    hip.close()

    batch = hip_lib.LvtBatch.create_mixed([q.prm, q.prm], 2)
    refused(batch, L.lvt_amd_set_depth_guard(batch._h, C.byref(bad["radius 4"])), "solo call on a batch")              # the spelling before the record
    refused(batch, batch.set_depth_guard(2, ok), "seq 2")
    refused(batch, batch.set_depth_guard(-1, bad["radius 4"]), "seq -1")                                                 # the sequence before the record
    refused(batch, batch.set_depth_guard(1, bad["support 25"]), "support 25")
    with pytest.raises(IndexError):
        batch.depth_guard_stats(2)
    with pytest.raises(IndexError):
        batch.depth_guard(2)
    assert batch.set_depth_guard(1, ok) == 0 and batch.depth_guard(0) is None and batch.depth_guard(1).radius == 2
    batch.close()

    kw, kprm, _ = make_case("kitti", 71, size=(621, 187))
    pair = tuple(np.ascontiguousarray(a) for a in kw.render_stereo(0))
    stereo = hip_lib.LvtSystem.create(kprm, 1)
    refused(stereo, stereo.set_depth_guard(ok), "stereo")
    refused(stereo, L.lvt_amd_batch_set_depth_guard(stereo._h, 3, C.byref(bad["radius 0"])), "stereo")                  # the sensor before the spelling
    assert stereo.depth_guard() is None and stereo.depth_guard_stats() is None
    sb = hip_lib.LvtBatch(kprm, 2)
    refused(sb, L.lvt_amd_set_depth_guard(sb._h, C.byref(ok)), "stereo")
    sb.close()
    seat = hip_lib.LvtSystem.create(kprm, 1, pooled=True)
    kprm.write_yaml(str(tmp_path / "cfg.yaml"))
    autos = [hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1) for _ in range(2)]
    assert seat.ordering() == "pooled" and autos[0].ordering() == "pooled"
    for h in (seat, autos[0]):
        refused(h, h.set_depth_guard(ok), "pooled")
        refused(h, L.lvt_amd_batch_set_depth_guard(h._h, 7, C.byref(bad["radius 0"])), "pooled")                        # the kind before everything
        assert h.depth_guard() is None and h.depth_guard_stats() is None
    for h in [stereo, seat, autos[0]]:
        h.track(*pair)
        assert h.get_state() == 2
    for h in [stereo, seat] + autos:
        h.close()
    assert set(seen) == set(TEXT), set(TEXT) - set(seen)
