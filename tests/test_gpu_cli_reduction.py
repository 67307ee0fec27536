"""examples/lvt_kitti --reduce F: the tracker is created at W / F x H / F with the reduced calibration and handed the decoded full-size PNGs.  The trajectory
file must be the one the program writes, WITHOUT the option, on the numpy-reduced PNGs with the reduced calibration -- byte for byte."""
import os
import subprocess

import pytest

import lvt_amd
import reduce_util as RU
from test_gpu_cli import _png

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "lvt_kitti")


def _dataset(root, frames, fx, fy, cx, cy, baseline):
    seq = root / "sequences" / "07"
    (seq / "image_0").mkdir(parents=True)
    (seq / "image_1").mkdir(parents=True)
    (root / "calib").mkdir()
    for i, (L, R) in enumerate(frames):
        _png(str(seq / "image_0" / f"{i:06d}.png"), L, filt=i % 4)
        _png(str(seq / "image_1" / f"{i:06d}.png"), R, filt=(i + 1) % 4)
    with open(root / "calib" / "07.yml", "w") as f:   # (repr: the shortest text that reads back as the same double)
        f.write("%%YAML:1.0\n\ncamera_matrix: !!opencv-matrix\n  rows: 3\n  cols: 3\n  dt: d\n  data: [ %r, 0, %r, 0, %r, %r, 0, 0, 1 ]\n\nbaseline: %r\n"
                % (float(fx), float(cx), float(fy), float(cy), float(baseline)))


def _run(root, *extra):
    out = subprocess.run([EXE, str(root / "sequences"), "7", "--config", str(root / "config.yaml"), "--calib", str(root / "calib" / "07.yml"),
                          "--out", str(root / "07.txt"), *extra], cwd=root, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return open(root / "07.txt", "rb").read()


@pytest.mark.parametrize("f,size", [(2, (1240, 376)), (3, (1241, 376))])
def test_kitti_cli_reduce_equals_the_cli_on_reduced_pngs(tmp_path, hip_lib, f, size):
    q = RU.large_world("kitti", 3, size, f)
    w, n = q.world, 5
    big, small = tmp_path / "big", tmp_path / "small"
    big.mkdir(); small.mkdir()
    _dataset(big, q.large[:n], w.fx, w.fy, w.cx, w.cy, w.baseline)
    _dataset(small, q.small[:n], *RU.reduced_intrinsics(w.fx, w.fy, w.cx, w.cy, f), w.baseline)
    for d in (big, small):
        lvt_amd.kitti_params().write_yaml(str(d / "config.yaml"))
    got, want = _run(big, "--reduce", str(f)), _run(small)
    assert len(want.splitlines()) == n
    assert got == want
