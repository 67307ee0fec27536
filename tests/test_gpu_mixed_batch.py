"""A MIXED lock-step batch (lvt_amd_batch_create_mixed): sequences with their own image size, intrinsics, detection grid, radii and thresholds
through ONE launch chain, each held to ITS OWN oracle instance: every pose within POSE_TOL, every state equal, all counters equal after the
last frame, no error."""
import ctypes

import numpy as np
import pytest

from case_tables import KITTI_DENSE_UNSTAGED, PNP_STAGE_MAX
from parity_util import make_case, pose_errors, POSE_TOL

pytestmark = pytest.mark.gpu

KITTI_00_07_SHAPES = [(1241, 376)] * 3 + [(1242, 375)] + [(1226, 370)] * 4   # drives 00 - 02, 03, 04 - 07


class Seq:
    """one sequence of a batch: its world's frames (rendered once), its parameters, its images in HBM"""

    def __init__(self, world, prm, n, first=0, edit=None):
        import torch
        self.prm, self.W, self.H, self.n = prm, world.W, world.H, n
        self.frames = [world.render_stereo(first + i) for i in range(n)]
        if edit:
            self.frames = [(edit(a), edit(b)) for a, b in self.frames]
        self.pitch = ((self.W + 63) // 64) * 64
        self.dev = torch.zeros((n, 2, self.H, self.pitch), dtype=torch.uint8, device="cuda")
        for i, (a, b) in enumerate(self.frames):
            self.dev[i, 0, :, :self.W] = torch.from_numpy(a).cuda(); self.dev[i, 1, :, :self.W] = torch.from_numpy(b).cuda()
        torch.cuda.synchronize()

    def ptrs(self, i):
        return self.dev[i, 0].data_ptr(), self.dev[i, 1].data_ptr()


def step(batch, seqs, which):
    """enqueue one lock-step step; which[s]: the frame of sequence s in it, None = absent"""
    lp = [None if i is None else q.ptrs(i)[0] for q, i in zip(seqs, which)]
    rp = [None if i is None else q.ptrs(i)[1] for q, i in zip(seqs, which)]
    return batch.track_device_async_mixed(lp, rp, [q.H for q in seqs], [q.W for q in seqs], [q.pitch for q in seqs])


def run(batch, seqs, schedule, depth=3):
    """schedule[k][s]: frame index or None; returns the per-step results (R, t, state), `depth` steps in flight"""
    got, inflight = [], 0
    for which in schedule:
        assert step(batch, seqs, which) == 0, batch.last_error()
        inflight += 1
        if inflight >= depth:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    return got


def check_against_own_oracles(batch, seqs, schedule, got, must_track=True):
    from oracle import pyoracle as O
    for s, q in enumerate(seqs):
        orc = O.Oracle(q.prm, 1)
        for k, which in enumerate(schedule):
            if which[s] is None:
                continue
            Ro, to = orc.track(*q.frames[which[s]])
            Rb, tb, st = got[k]
            e_t, e_R = pose_errors(Rb[s], tb[s], Ro, to)
            print(f"sequence {s} step {k} frame {which[s]}: e_t {e_t:.2e} e_R {e_R:.2e} state {st[s]} / {orc.status}")
            assert e_t <= POSE_TOL and e_R <= POSE_TOL and st[s] == orc.status, f"sequence {s} step {k}: {e_t:.2e} {e_R:.2e} state {st[s]} oracle {orc.status}"
            if must_track:
                assert orc.status == 2, f"sequence {s} step {k}: the oracle is not TRACKING"
        co, ch = orc.counts(), batch.counts(s)
        bad = {k: (ch.get(k), v) for k, v in co.items() if ch.get(k) != v}
        assert not bad, f"sequence {s}: counters (hip, oracle) {bad}"


def test_kitti_00_07_shapes_in_one_batch(hip_lib, oracle_lib):
    """eight sequences with the three image sizes of KITTI 00 - 07, each with its world's own intrinsics, 24 frames, three steps in flight"""
    n = 24
    seqs = []
    for s, size in enumerate(KITTI_00_07_SHAPES):
        world, prm, _ = make_case("kitti", 60 + s, 1.0, None, size=size)
        seqs.append(Seq(world, prm, n))
    assert len({(q.prm.fx, q.W, q.H) for q in seqs}) == 3
    batch = hip_lib.LvtBatch.create_mixed([q.prm for q in seqs])
    assert batch.B == 8 and hip_lib.load_library().lvt_amd_batch_size(batch._h) == 8
    for s, q in enumerate(seqs):
        assert bytes(batch.params(s).to_pod()) == bytes(q.prm.to_pod())
    schedule = [[i] * 8 for i in range(n)]
    got = run(batch, seqs, schedule)
    assert batch.last_error() == "", batch.last_error()
    check_against_own_oracles(batch, seqs, schedule, got)


def test_everything_different_in_one_batch(hip_lib, oracle_lib):
    """one step mixes staged / unstaged configurations, strip kernels / none, both list routes, three cell_search_radius values, five image sizes"""
    n = 12
    patch = np.random.default_rng(5).integers(0, 256, size=(257, 257), dtype=np.uint8)

    def patched(img):   # a noise patch over cell 0: more raw corners than one workgroup's LDS holds -> the strip kernels (test_gpu_parity.py, strips_257)
        img = img.copy()
        img[:257, :257] = patch
        return img
    cases = [  # (kind, seed, size, overrides, edit) -- the strips sequence FIRST: the debug stamps read below are sequence 0's
        ("kitti", 33, (1241, 376), {"detection_cell_size": 257}, patched),
        ("kitti", 34, (1241, 376), {}, None),
        ("kitti", 33, (1241, 376), {"detection_cell_size": 100, "max_keypoints_per_cell": 40}, None),
        ("kitti", 32, (620, 188), {"tracking_radius": 75}, None),
        ("kitti", 36, (1280, 720), {}, None),
        ("euroc", 3, None, {}, None),                    # 752 x 480: staged_threshold 0, a 2-px last grid column
    ]
    seqs = []
    for kind, seed, size, over, edit in cases:
        world, prm, _ = make_case(kind, seed, 1.0, over, size=size)
        seqs.append(Seq(world, prm, n, edit=edit))
    assert (seqs[5].W, seqs[5].H, seqs[5].prm.staged_threshold) == (752, 480, 0)
    batch = hip_lib.LvtBatch([q.prm for q in seqs])
    schedule = [[i] * len(seqs) for i in range(n)]
    got = run(batch, seqs, schedule)
    assert batch.last_error() == "", batch.last_error()
    stamps = np.zeros(32, np.int64)   # cell 0 of sequence 0's left image in the last frame really took the strip route
    hip_lib.load_library().lvt_amd_get_debug(batch._h, stamps.ctypes.data_as(ctypes.c_void_p))
    assert int(stamps[10]) in (1001, 1002), int(stamps[10])
    check_against_own_oracles(batch, seqs, schedule, got)


def test_staged_and_unstaged_solve_in_one_launch(hip_lib, oracle_lib):
    """one world twice in a batch: under the dense parameters (more than PNP_STAGE_MAX matches from frame 2 on: k_pnp's edges stay in global
    memory) and under the defaults (about 600 matches, staged in LDS) -- one k_pnp launch holds both kinds of solve, three steps in flight"""
    _, kind, seed, scale, overrides, frames = KITTI_DENSE_UNSTAGED
    world, prm_dense, _ = make_case(kind, seed, scale, overrides)
    _, prm_default, _ = make_case(kind, seed, scale)
    seqs = [Seq(world, prm_dense, len(frames)), Seq(world, prm_default, len(frames))]
    batch = hip_lib.LvtBatch([prm_dense, prm_default])
    schedule = [[i, i] for i in frames]
    got = run(batch, seqs, schedule)
    assert batch.last_error() == "", batch.last_error()
    check_against_own_oracles(batch, seqs, schedule, got)
    assert batch.counts(0)["n_matches"] > PNP_STAGE_MAX and 0 < batch.counts(1)["n_matches"] <= PNP_STAGE_MAX, (batch.counts(0), batch.counts(1))


def test_sequences_of_different_lengths(hip_lib, oracle_lib):
    """6 / 14 / 20 frames in one batch of 20 steps: a sequence without a frame in a step is passed as None -- at its end, and in a MIDDLE step --
    and is left exactly as it is: previous pose and state, counters (frame number included) unchanged"""
    lens = (6, 14, 20)
    sizes = ((620, 188), (621, 187), (613, 185))
    seqs = []
    for s, (m, size) in enumerate(zip(lens, sizes)):
        world, prm, _ = make_case("kitti", 70 + s, 1.0, None, size=size)
        seqs.append(Seq(world, prm, m))
    hole = 7                                   # the step sequence 1 sits out in the middle of its drive
    schedule, nxt = [], [0, 0, 0]
    for k in range(20):
        which = []
        for s in range(3):
            if nxt[s] < lens[s] and not (s == 1 and k == hole):
                which.append(nxt[s]); nxt[s] += 1
            else:
                which.append(None)
        schedule.append(which)
    assert nxt == list(lens) and schedule[hole][1] is None and schedule[hole + 1][1] == hole
    batch = hip_lib.LvtBatch.create_mixed([q.prm for q in seqs])
    got, inflight = [], 0
    for k, which in enumerate(schedule):
        if k == hole:                          # drain, so that counts() speaks of step hole - 1 and then of step hole
            while inflight:
                got.append(batch.wait()); inflight -= 1
            before = batch.counts(1)
        assert step(batch, seqs, which) == 0, batch.last_error()
        inflight += 1
        if k == hole:
            got.append(batch.wait()); inflight -= 1
            assert batch.counts(1) == before and before["frame"] == hole - 1, (before, batch.counts(1))
        elif inflight >= 3:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    assert batch.last_error() == "", batch.last_error()
    for k in range(1, 20):                     # an absent step returns the previous step's pose and state
        for s in range(3):
            if schedule[k][s] is None:
                # (both are fp64 conversions of the one pose the tracker holds: equal to rounding)
                assert np.allclose(got[k][0][s], got[k - 1][0][s], rtol=0, atol=1e-12) and np.allclose(got[k][1][s], got[k - 1][1][s], rtol=0, atol=1e-12), (k, s)
                assert got[k][2][s] == got[k - 1][2][s], (k, s)
    check_against_own_oracles(batch, seqs, schedule, got)   # (the counters of sequence 0 are still those of its frame 5 after 14 steps without it)
    assert [batch.counts(s)["frame"] for s in range(3)] == [m - 1 for m in lens]


def test_a_sequence_absent_on_alternate_steps(hip_lib, oracle_lib):
    """three sequences, RING + 2 = 10 steps, sequence 1 sits out every other one: its input record of a ring slot says "absent" where the slot's
    previous step left planes and the other way round, and each sequence still equals its own oracle"""
    steps = 8 + 2
    sizes = ((620, 188), (621, 187), (613, 185))
    seqs = []
    for s, size in enumerate(sizes):
        world, prm, _ = make_case("kitti", 70 + s, 1.0, None, size=size)
        seqs.append(Seq(world, prm, steps // 2 if s == 1 else steps))
    schedule = [[k, k // 2 if k % 2 == 0 else None, k] for k in range(steps)]
    batch = hip_lib.LvtBatch.create_mixed([q.prm for q in seqs])
    got = run(batch, seqs, schedule)
    assert batch.last_error() == "", batch.last_error()
    for k in range(1, steps, 2):   # an absent step returns the previous step's pose and state
        assert np.allclose(got[k][0][1], got[k - 1][0][1], rtol=0, atol=1e-12) and np.allclose(got[k][1][1], got[k - 1][1][1], rtol=0, atol=1e-12), k
        assert got[k][2][1] == got[k - 1][2][1], k
    check_against_own_oracles(batch, seqs, schedule, got)
    assert [batch.counts(s)["frame"] for s in range(3)] == [steps - 1, steps // 2 - 1, steps - 1]


def test_uniform_equals_mixed_bit_for_bit(hip_lib):
    """the same three sequences under one parameter set through LvtBatch(prm, 3) and through the mixed constructor: identical poses, states, counters"""
    n = 12
    world, prm, _ = make_case("kitti", 32, 1.0, None, size=(620, 188))
    seqs = [Seq(world, prm, n, first=2 * s) for s in range(3)]
    uni = hip_lib.LvtBatch(prm, 3)
    got_u, inflight = [], 0
    for i in range(n):
        uni.track_device_async([q.ptrs(i)[0] for q in seqs], [q.ptrs(i)[1] for q in seqs], seqs[0].H, seqs[0].W, seqs[0].pitch)
        inflight += 1
        if inflight >= 3:
            got_u.append(uni.wait()); inflight -= 1
    while inflight:
        got_u.append(uni.wait()); inflight -= 1
    mix = hip_lib.LvtBatch([prm, prm, prm])
    got_m = run(mix, seqs, [[i] * 3 for i in range(n)])
    assert uni.last_error() == "" and mix.last_error() == ""
    for i in range(n):
        for a, b in zip(got_u[i], got_m[i]):
            assert (a == b).all(), f"frame {i}"
    assert (got_u[-1][2] == 2).all()
    for s in range(3):
        assert uni.counts(s) == mix.counts(s), s


def test_rejections_enqueue_nothing(hip_lib, oracle_lib):
    world0, prm0, _ = make_case("kitti", 32, 1.0, None, size=(620, 188))
    world1, prm1, _ = make_case("kitti", 71, 1.0, None, size=(621, 187))
    seqs = [Seq(world0, prm0, 6), Seq(world1, prm1, 6)]
    batch = hip_lib.LvtBatch.create_mixed([prm0, prm1])
    got = run(batch, seqs, [[0, 0], [1, 1]])
    enq = batch.host_stats()["enqueued"]
    assert enq == 2
    H, W, P = [q.H for q in seqs], [q.W for q in seqs], [q.pitch for q in seqs]
    lp, rp = [q.ptrs(2)[0] for q in seqs], [q.ptrs(2)[1] for q in seqs]
    assert batch.track_device_async_mixed(lp, rp, H, [W[0], W[0]], P) == -1           # sequence 1 handed sequence 0's width
    assert "sequence 1" in batch.last_error(), batch.last_error()
    assert batch.track_device_async_mixed(lp, rp, [H[0] + 1, H[1]], W, P) == -1
    assert "sequence 0" in batch.last_error(), batch.last_error()
    assert batch.track_device_async_mixed(lp, rp, H, W, [P[0], P[1] + 8]) == -1         # a pitch that is not a multiple of 16
    assert "sequence 1" in batch.last_error(), batch.last_error()
    assert batch.track_device_async_mixed([None, None], [None, None], H, W, P) == -1
    assert "no sequence" in batch.last_error(), batch.last_error()
    assert batch.host_stats()["enqueued"] == enq
    schedule = [[i, i] for i in range(6)]
    got += run(batch, seqs, schedule[2:])                                                # the next valid steps track as if nothing had happened
    check_against_own_oracles(batch, seqs, schedule, got)
    # a refused parameter set (65 detection cells) refuses the whole batch
    _, bad, _ = make_case("kitti", 0, 1.0, {"detection_cell_size": 100})
    bad.img_width, bad.img_height = 1241, 420
    with pytest.raises(Exception):
        hip_lib.LvtBatch.create_mixed([prm0, bad])
    L = hip_lib.load_library()
    pods = (hip_lib.ParamsPOD * 2)(prm0.to_pod(), bad.to_pod())
    assert not L.lvt_amd_batch_create_mixed(pods, 1, 2)
    # the batch entry points on a handle that is not a batch context: they return
    cfg = _yaml(prm0)
    L.lvt_create.restype = ctypes.c_void_p
    h = L.lvt_create(cfg.encode(), 1)
    assert h
    assert L.lvt_amd_batch_size(ctypes.c_void_p(h)) in (0, 1)
    out = hip_lib.ParamsPOD()
    assert L.lvt_amd_batch_get_params(ctypes.c_void_p(h), 5, ctypes.byref(out)) == 0
    L.lvt_destroy(ctypes.c_void_p(h))


def _yaml(prm):
    import os
    import tempfile
    d = tempfile.mkdtemp()
    path = os.path.join(d, "cfg.yaml")
    prm.write_yaml(path)
    return path
