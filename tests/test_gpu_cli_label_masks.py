"""examples/lvt_kitti --labels DIR --drop L1,L2 --dilate R: the label files are read through the PNG reader of examples/image_io.h and handed to the tracker
frame by frame.  The trajectory is held FIRST against the oracle's route for a masked frame (mask_util) under that frame's numpy plane (label_mask_util),
then -- tighter, as a plumbing check -- against the Python binding with the same labels.  A frame whose file is missing gets no labels."""
import subprocess

import numpy as np
import pytest

import label_mask_util as LU
import mask_util as MU
from test_gpu_cli import _png, _se3_close
from test_gpu_cli_masks import _exe, _pgm

pytestmark = pytest.mark.gpu


def test_kitti_cli_with_labels(tmp_path):
    import lvt_amd
    from lvt_amd.synth import make_world
    from oracle import pyoracle as O
    exe = _exe("lvt_kitti")
    world = make_world("kitti", seed=3, scale=0.5)
    prm = lvt_amd.kitti_params(width=world.W, height=world.H, fx=world.fx, fy=world.fy, cx=world.cx, cy=world.cy, baseline=world.baseline)
    seq = tmp_path / "sequences" / "07"
    for d in (seq / "image_0", seq / "image_1", tmp_path / "calib", tmp_path / "labels"):
        d.mkdir(parents=True)
    n, missing, dilate = 6, 3, 3
    frames = [tuple(np.ascontiguousarray(a) for a in world.render_stereo(i)) for i in range(n)]
    size = LU.label_sizes(world.W, world.H)["quarter"]
    labs, masks = LU.sliding_masks(world.W, world.H, size, dilate, n=n)
    masks[missing] = None
    for i, (L, R) in enumerate(frames):
        _png(str(seq / "image_0" / f"{i:06d}.png"), L, filt=i % 4)
        _pgm(str(seq / "image_1" / f"{i:06d}.pgm"), R)
        if i != missing:
            _png(str(tmp_path / "labels" / f"{i:06d}.png"), labs[i], filt=(i + 1) % 4)
    with open(tmp_path / "calib" / "07.yml", "w") as f:
        f.write("%%YAML:1.0\n\ncamera_matrix: !!opencv-matrix\n  rows: 3\n  cols: 3\n  dt: d\n  data: [ %.12e, 0, %.12e, 0, %.12e, %.12e, 0, 0, 1 ]\n\nbaseline: %.10e\n"
                % (prm.fx, prm.cx, prm.fy, prm.cy, prm.baseline))
    prm.write_yaml(str(tmp_path / "vo_config.yaml"))
    base = [exe, str(tmp_path / "sequences"), "7", "--labels", str(tmp_path / "labels")]

    bad = subprocess.run(base + ["--drop", "11,13", "--dilate", "16", "--out", "bad.txt"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "dilate = 16 (0 ... 15)" in bad.stdout and not (tmp_path / "bad.txt").exists(), bad.stdout + bad.stderr
    gone = subprocess.run([exe, str(tmp_path / "sequences"), "7", "--labels", str(tmp_path / "nothing"), "--drop", "11"], cwd=tmp_path, capture_output=True, text=True,
                          timeout=300)
    assert gone.returncode != 0 and "failed to read the labels" in gone.stdout, gone.stdout + gone.stderr

    out = subprocess.run(base + ["--drop", ",".join(str(l) for l in LU.DROPPED), "--dilate", str(dilate)], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    traj = np.loadtxt(tmp_path / "07.txt").reshape(-1, 3, 4)
    assert traj.shape[0] == n
    file_prm = lvt_amd.LvtParameters.from_file(str(tmp_path / "vo_config.yaml"))
    orc = O.Oracle(file_prm, 1)
    for i, (L, R) in enumerate(frames):
        Ro, to, _ = MU.oracle_track_masked(orc, file_prm, L, R, masks[i], None, f"frame {i}", 0.10 if masks[i] is not None else 0.0)
        assert orc.status == 2
        _se3_close(traj[i, :, :3], traj[i, :, 3], Ro, to, f"lvt_kitti --labels frame {i}")
    ref = lvt_amd.LvtSystem.create_from_file(str(tmp_path / "vo_config.yaml"), lvt_amd.eSensor_STEREO)
    assert ref.set_label_mask(lvt_amd.LabelMask(size[0], size[1], LU.DROPPED, dilate)) == 0, ref.last_error()
    plain = lvt_amd.LvtSystem.create(file_prm, 1)
    differs = False
    for i, (L, R) in enumerate(frames):
        if masks[i] is not None:
            assert ref.frame_labels(labs[i], None) == 0, ref.last_error()
        Rm, t = ref.track(L, R)
        Rp, tp = plain.track(L, R)
        differs = differs or not np.array_equal(t, tp)
        assert ref.get_state() == 2 and (ref.mask_stats() is None) == (masks[i] is None)
        assert np.allclose(traj[i, :, :3], Rm, atol=2e-9) and np.allclose(traj[i, :, 3], t, atol=2e-9), f"frame {i}"
    assert differs, "the labelled trajectory is the plain one: the comparison shows nothing"
