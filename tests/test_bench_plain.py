"""CPU tier: what a plain `bench.py` run does besides the timed steps -- the frame each step tracks (rendering does not grow with
--steps, and runs of up to FRAMES_RENDERED_MAX steps track the frames they always did), the side legs off unless --full, and
--dump-outputs (the last timed step's arrays as float64 .npy, written before any side leg runs on the handle)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from lvt_amd.shard import RankEnv  # noqa: E402


def test_frame_order_is_the_sequence_then_a_continuous_walk_over_the_rendered_frames():
    n = bench.FRAMES_RENDERED_MAX
    order = [bench.frame_index(i) for i in range(5 * n)]
    assert order[:n] == list(range(n))
    assert min(order) == 0 and max(order) == n - 1
    assert all(abs(a - b) == 1 for a, b in zip(order, order[1:]))   # no jump anywhere: the camera path stays continuous


def test_side_legs_are_off_by_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and a.dump_outputs == ""
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full is True


class _Backend:
    sequences_per_gpu = 1
    workload = "stand-in"

    def __init__(self):
        self.log = []

    def sync(self):
        pass

    def prepare(self, n):
        pass

    def warmup(self, Wm):
        return [None] * Wm

    def timed(self, first, K, depth):
        self.log.append("timed")
        return [(None, None)] * K, 0

    def outputs(self):
        self.log.append("outputs")
        return {"pose_R": np.eye(3, dtype=np.float32), "pose_t": np.arange(3), "tracking_state": 2}

    def extras(self, args, env, warm, poses):
        self.log.append("extras")
        return {}


def test_dump_outputs_writes_the_last_step_as_float64_before_the_side_legs(tmp_path):
    d = tmp_path / "out"
    args = bench.parse_args(["--steps", "4", "--warmup", "1", "--dump-outputs", str(d)])
    be = _Backend()
    res = bench.run_rank(args, RankEnv(0, 0, 1), None, be)
    assert res["steps"] == 4 and res["ms_per_step"] >= 0
    assert be.log == ["timed", "outputs", "extras"]
    got = {p: np.load(d / p) for p in sorted(os.listdir(d))}
    assert sorted(got) == ["pose_R.npy", "pose_t.npy", "tracking_state.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["pose_R.npy"], np.eye(3)) and np.array_equal(got["pose_t.npy"], [0, 1, 2]) and got["tracking_state.npy"] == 2
