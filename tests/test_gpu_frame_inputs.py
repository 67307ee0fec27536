"""Where a frame's planes lie is the frame's own: the feature stage publishes image pointers and pitch per frame into the feature buffer's control block
(FeatCtl::in, lvt_dev.h) and every later feature kernel reads them there.  Here consecutive frames sit in allocations of their own at two alternating
pitches, over 2 NPAR + 1 frames with three in flight, so every feature buffer is used by frames of both pitches: a pointer or pitch left over from the
buffer's previous frame would shear the image.  Each run is held to the oracle frame by frame."""
import pytest

from parity_util import make_case, pose_errors, diff_frame, POSE_TOL
from test_gpu_mixed_batch import check_against_own_oracles

pytestmark = pytest.mark.gpu

NPAR = 3   # lvt_dev.h
N = 2 * NPAR + 1


class Planes:
    """one sequence: its frames (rendered once) and, per frame, a stereo pair in an allocation of its own at that frame's pitch"""

    def __init__(self, world, prm, n, pitch_of, first=0):
        import torch
        self.prm, self.W, self.H = prm, world.W, world.H
        self.frames = [world.render_stereo(first + i) for i in range(n)]
        self.pitch = [pitch_of(i) for i in range(n)]
        self.dev = []
        for (a, b), p in zip(self.frames, self.pitch):
            d = torch.zeros((2, self.H, p), dtype=torch.uint8, device="cuda")
            d[0, :, :self.W] = torch.from_numpy(a).cuda(); d[1, :, :self.W] = torch.from_numpy(b).cuda()
            self.dev.append(d)
        torch.cuda.synchronize()
        assert len({d.data_ptr() for d in self.dev}) == n

    def ptrs(self, i):
        return self.dev[i][0].data_ptr(), self.dev[i][1].data_ptr()


def alternating(W):
    base = ((W + 63) // 64) * 64
    return lambda i: base + 64 * (i % 2)


def test_planes_at_a_changing_pitch_and_address(hip_lib, oracle_lib):
    """one stereo handle through lvt_amd_track_device_async: k_score<true> takes the planes from its arguments, k_brief's border fall-back from the record"""
    world, prm, _ = make_case("kitti", 8, 0.5)
    q = Planes(world, prm, N, alternating(world.W))
    assert len(set(q.pitch)) == 2
    hip = hip_lib.LvtSystem.create(prm, 1)
    orc = oracle_lib.Oracle(prm, 1)
    got, inflight = [], 0
    for i in range(N):
        hip.track_device_async(*q.ptrs(i), q.H, q.W, q.pitch[i])
        inflight += 1
        if inflight >= 3:
            got.append(hip.wait_status()); inflight -= 1
    while inflight:
        got.append(hip.wait_status()); inflight -= 1
    for i, (a, b) in enumerate(q.frames):
        Ro, to = orc.track(a, b)
        Rh, th, st = got[i]
        e_t, e_R = pose_errors(Rh, th, Ro, to)
        print(f"frame {i} (pitch {q.pitch[i]}): e_t {e_t:.2e} e_R {e_R:.2e} state {st} / {orc.status}")
        assert e_t <= POSE_TOL and e_R <= POSE_TOL and st == orc.status, f"frame {i} (pitch {q.pitch[i]}): e_t {e_t:.2e} e_R {e_R:.2e} state {st} / {orc.status}"
    msgs = diff_frame(hip, orc)
    assert not msgs, msgs[:6]
    assert hip.last_error() == "", hip.last_error()


def _run_uniform(batch, seqs, n, pitch_of):
    got, inflight = [], 0
    for i in range(n):
        batch.track_device_async([q.ptrs(i)[0] for q in seqs], [q.ptrs(i)[1] for q in seqs], seqs[0].H, seqs[0].W, pitch_of(i))
        inflight += 1
        if inflight >= 3:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    assert batch.last_error() == "", batch.last_error()
    return got


def test_batch_planes_at_a_changing_pitch_and_address(hip_lib, oracle_lib):
    """the same schedule on a uniform batch of two (lvt_amd_batch_track_device_async), the pitch alternating per step: k_feat_begin_pack writes the record,
    k_score<false> reads planes and pitch from it; each sequence against its own oracle"""
    world, prm, _ = make_case("kitti", 8, 0.5)
    pitch_of = alternating(world.W)
    seqs = [Planes(world, prm, N, pitch_of, first=2 * s) for s in range(2)]
    batch = hip_lib.LvtBatch(prm, 2)
    got = _run_uniform(batch, seqs, N, pitch_of)
    check_against_own_oracles(batch, seqs, [[i, i] for i in range(N)], got)


def test_batch_brief_without_the_box_sum_plane(hip_lib, oracle_lib, monkeypatch):
    """LVT_AMD_BRIEF_FROM_IMAGE=1 on a uniform batch of two: k_brief_img<false> reads the image through the record for every key point (the single handle:
    test_gpu_parity.test_brief_without_the_box_sum_plane); each sequence against its own oracle"""
    monkeypatch.setenv("LVT_AMD_BRIEF_FROM_IMAGE", "1")
    n = 4
    world, prm, _ = make_case("kitti", 8, 0.5)
    pitch = ((world.W + 63) // 64) * 64
    seqs = [Planes(world, prm, n, lambda i: pitch, first=2 * s) for s in range(2)]
    batch = hip_lib.LvtBatch(prm, 2)
    got = _run_uniform(batch, seqs, n, lambda i: pitch)
    check_against_own_oracles(batch, seqs, [[i, i] for i in range(n)], got)
