"""Helpers of the RGB-D GPU tests (test_gpu_rgbd_batch.py, test_gpu_rgbd_edges.py): sequences with their planes in HBM, frame records, lock-step batch
drivers.  16-bit depth u = clip(rint(d * 5000), 0, 65535) as uint16, scale s = float32(1) / float32(5000)."""
import numpy as np

from parity_util import make_case, pose_errors, diff_frame, POSE_TOL

SCALE = np.float32(1) / np.float32(5000)


def need(hip_lib, *names):
    L = hip_lib.load_library()
    for n in names:
        assert hasattr(L, n), f"liblvt_c.so does not export {n}"
        assert hasattr(getattr(L, n), "argtypes") and getattr(L, n).argtypes, f"{n} has no ctypes signature in lvt_amd"
    return L


def quantise(d):
    return np.clip(np.rint(d.astype(np.float64) * 5000.0), 0, 65535).astype(np.uint16)


def patch(u):
    H, W = u.shape
    u = u.copy()
    u[H * 5 // 24: H * 25 // 48, W * 5 // 32: W * 15 // 32] = 0          # no depth
    u[H * 5 // 8: H * 5 // 6, W * 5 // 8: W * 15 // 16] = 30000           # 6 m: beyond far_plane_distance 5.0
    return u


class RSeq:
    """one RGB-D sequence: gray frames, 16-bit depth u, its fp32 conversion u * s (what the oracle and every fp32 entry get); in HBM: the gray planes,
    the fp32 planes with a row pitch LARGER than the row, and the 16-bit planes at a 2-byte-but-not-4-byte aligned address with a padded pitch"""

    def __init__(self, seed, overrides, size, n, first=0, patched=False, device=True):
        self.world, self.prm, sensor = make_case("tum", seed, 1.0, overrides, size)
        assert sensor == 2
        self.W, self.H, self.n = self.world.W, self.world.H, n
        self.gray, self.u16, self.f32 = [], [], []
        for i in range(n):
            g, d = self.world.render_rgbd(first + i)
            u = quantise(d)
            assert int(u.max()) <= 22500, int(u.max())
            if patched:
                u = patch(u)
            self.gray.append(np.ascontiguousarray(g)); self.u16.append(u); self.f32.append(u.astype(np.float32) * SCALE)
            assert self.f32[-1].dtype == np.float32
        if device:
            self.to_device()

    @classmethod
    def from_frames(cls, prm, gray, f32, u16=None, device=True):
        """the same holder around frames made elsewhere: fp32 planes of any content (NaN and infinities included), 16-bit planes only where the frames
        have them (then f32 must be their conversion under the scale the test tracks them with)"""
        q = cls.__new__(cls)
        q.world, q.prm = None, prm
        q.H, q.W = gray[0].shape
        q.n = len(gray)
        q.gray = [np.ascontiguousarray(g, dtype=np.uint8) for g in gray]
        q.f32 = [np.ascontiguousarray(d, dtype=np.float32) for d in f32]
        q.u16 = None if u16 is None else [np.ascontiguousarray(u, dtype=np.uint16) for u in u16]
        assert len(q.f32) == q.n and (q.u16 is None or len(q.u16) == q.n)
        if device:
            q.to_device()
        return q

    def to_device(self):
        import torch
        n, H, W = self.n, self.H, self.W
        self.gpitch = ((W + 63) // 64) * 64
        self.fpitch_el = W + 12           # fp32 rows padded by 12 elements
        self.upitch_el = W + 6            # 16-bit rows padded by 6 elements
        self.d_gray = torch.zeros((n, H, self.gpitch), dtype=torch.uint8, device="cuda")
        self.d_f32 = torch.full((n, H, self.fpitch_el), 3.0, dtype=torch.float32, device="cuda")
        self.d_f32_tight = torch.zeros((n, H, W), dtype=torch.float32, device="cuda")
        self.u_plane = H * self.upitch_el + 2                                    # (even: every frame keeps the odd element offset)
        self.d_u16_flat = torch.full((n * self.u_plane + 2,), 15000, dtype=torch.int16, device="cuda")
        for i in range(n):
            self.d_gray[i, :, :W] = torch.from_numpy(self.gray[i]).cuda()
            self.d_f32[i, :, :W] = torch.from_numpy(self.f32[i]).cuda()
            self.d_f32_tight[i] = torch.from_numpy(self.f32[i]).cuda()
            if self.u16 is not None:
                v = self.d_u16_flat[1 + i * self.u_plane: 1 + i * self.u_plane + H * self.upitch_el].view(H, self.upitch_el)
                v[:, :W] = torch.from_numpy(self.u16[i].view(np.int16)).cuda()
        torch.cuda.synchronize()
        assert self.u16_ptr(0) % 4 == 2

    def gray_ptr(self, i):
        return self.d_gray[i].data_ptr()

    def f32_ptr(self, i, tight=False):
        return (self.d_f32_tight if tight else self.d_f32)[i].data_ptr()

    def f32_pitch(self, tight=False):
        return 4 * (self.W if tight else self.fpitch_el)

    def u16_ptr(self, i):
        return self.d_u16_flat.data_ptr() + 2 * (1 + i * self.u_plane)

    def u16_pitch(self):
        return 2 * self.upitch_el


def record(sys_, R, t):
    return (R.copy(), t.copy(), sys_.get_state(), sys_.counts(), sys_.features(0))


def same_records(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), f"{what}: pose differs at frame {i}"
        assert x[2] == y[2], f"{what}: state differs at frame {i}"
        assert x[3] == y[3], f"{what}: counters differ at frame {i}: {x[3]} / {y[3]}"
        for k in range(3):
            assert np.array_equal(x[4][k], y[4][k]), f"{what}: features(0)[{k}] differ at frame {i}"


def run_host_f32(hip_lib, q, orc=None):
    """the fp32 host entry (lvt_amd_track_rgbd), frame by frame; with an oracle: diffed against it, which must be TRACKING throughout"""
    sys_ = hip_lib.LvtSystem.create(q.prm, 2)
    out = []
    for i in range(q.n):
        R, t = sys_.track(q.gray[i], q.f32[i])
        if orc is not None:
            Ro, to = orc.track_rgbd(q.gray[i], q.f32[i])
            msgs = diff_frame(sys_, orc)
            e_t, e_R = pose_errors(R, t, Ro, to)
            print(f"frame {i}: e_t {e_t:.2e} e_R {e_R:.2e} n_left {sys_.counts()['n_left']} state {orc.status}")
            assert not msgs, f"frame {i}: {msgs}"
            assert e_t <= POSE_TOL and e_R <= POSE_TOL, f"frame {i}: {e_t:.2e} {e_R:.2e}"
            assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        out.append(record(sys_, R, t))
    assert sys_.last_error() == "", sys_.last_error()
    return out


def batch_step(batch, seqs, which, fmt, hip_lib):
    g = [None if i is None else q.gray_ptr(i) for q, i in zip(seqs, which)]
    if fmt == hip_lib.DEPTH_U16:
        d = [None if i is None else q.u16_ptr(i) for q, i in zip(seqs, which)]
        dp = [q.u16_pitch() for q in seqs]
    else:
        d = [None if i is None else q.f32_ptr(i) for q, i in zip(seqs, which)]
        dp = [q.f32_pitch() for q in seqs]
    return batch.track_rgbd_device_async(g, d, [q.H for q in seqs], [q.W for q in seqs], [q.gpitch for q in seqs], dp, fmt, SCALE)


def batch_run(batch, seqs, schedule, fmts, hip_lib, depth=3):
    got, inflight = [], 0
    for which, fmt in zip(schedule, fmts):
        assert batch_step(batch, seqs, which, fmt, hip_lib) == 0, batch.last_error()
        inflight += 1
        if inflight >= depth:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    return got


def check_against_own_oracles(oracle_lib, batch, seqs, schedule, got):
    for s, q in enumerate(seqs):
        orc = oracle_lib.Oracle(q.prm, 2)
        for k, which in enumerate(schedule):
            if which[s] is None:
                continue
            Ro, to = orc.track_rgbd(q.gray[which[s]], q.f32[which[s]])
            Rb, tb, st = got[k]
            e_t, e_R = pose_errors(Rb[s], tb[s], Ro, to)
            print(f"sequence {s} step {k} frame {which[s]}: e_t {e_t:.2e} e_R {e_R:.2e} state {st[s]} / {orc.status}")
            assert e_t <= POSE_TOL and e_R <= POSE_TOL and st[s] == orc.status, f"sequence {s} step {k}: {e_t:.2e} {e_R:.2e} state {st[s]} oracle {orc.status}"
            assert orc.status == 2, f"sequence {s} step {k}: the oracle is not TRACKING"
        co, ch = orc.counts(), batch.counts(s)
        bad = {k: (ch.get(k), v) for k, v in co.items() if ch.get(k) != v}
        assert not bad, f"sequence {s}: counters (hip, oracle) {bad}"
