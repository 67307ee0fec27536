"""examples/lvt_kitti --mask and examples/lvt_tum --mask: the mask files are read through the readers of examples/image_io.h and handed to the tracker before
the first frame.  The trajectory is held FIRST against the oracle's route for a masked frame (mask_util), then -- tighter, as a plumbing check -- against the
Python binding with the same mask.  A mask of another size is refused with a message and a non-zero exit before any frame is tracked."""
import os
import subprocess

import numpy as np
import pytest

import mask_util as MU
from test_gpu_cli import _png, _png16, _se3_close, _quat_xyzw_to_R, ROOT

pytestmark = pytest.mark.gpu


def _exe(name):
    exe = os.path.join(ROOT, "examples", name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s"])
    return exe


def _pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + np.ascontiguousarray(img).tobytes())


def test_kitti_cli_with_masks(tmp_path):
    import lvt_amd
    from lvt_amd.synth import make_world
    from oracle import pyoracle as O
    exe = _exe("lvt_kitti")
    world = make_world("kitti", seed=3, scale=0.5)
    prm = lvt_amd.kitti_params(width=world.W, height=world.H, fx=world.fx, fy=world.fy, cx=world.cx, cy=world.cy, baseline=world.baseline)
    seq = tmp_path / "sequences" / "07"
    (seq / "image_0").mkdir(parents=True)
    (seq / "image_1").mkdir(parents=True)
    (tmp_path / "calib").mkdir()
    n = 5
    frames = [tuple(np.ascontiguousarray(a) for a in world.render_stereo(i)) for i in range(n)]
    for i, (L, R) in enumerate(frames):
        _png(str(seq / "image_0" / f"{i:06d}.png"), L, filt=i % 4)
        _pgm(str(seq / "image_1" / f"{i:06d}.pgm"), R)
    with open(tmp_path / "calib" / "07.yml", "w") as f:
        f.write("%%YAML:1.0\n\ncamera_matrix: !!opencv-matrix\n  rows: 3\n  cols: 3\n  dt: d\n  data: [ %.12e, 0, %.12e, 0, %.12e, %.12e, 0, 0, 1 ]\n\nbaseline: %.10e\n"
                % (prm.fx, prm.cx, prm.fy, prm.cy, prm.baseline))
    prm.write_yaml(str(tmp_path / "vo_config.yaml"))
    ml, mr = MU.bonnet(world.W, world.H), MU.ellipse(world.W, world.H)
    _png(str(tmp_path / "left.png"), ml, filt=2)      # a PNG and a PGM: both readers
    _pgm(str(tmp_path / "right.pgm"), mr)
    _pgm(str(tmp_path / "small.pgm"), ml[:-1])

    bad = subprocess.run([exe, str(tmp_path / "sequences"), "7", "--mask", f"{tmp_path / 'left.png'},{tmp_path / 'small.pgm'}", "--out", "bad.txt"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "small.pgm is" in bad.stdout and f"the frames are {world.W} x {world.H}" in bad.stdout, bad.stdout + bad.stderr
    assert not (tmp_path / "bad.txt").exists(), "a trajectory was written behind a refused mask"
    gone = subprocess.run([exe, str(tmp_path / "sequences"), "7", "--mask", str(tmp_path / "nothing.png")], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert gone.returncode != 0 and "failed to read the mask" in gone.stdout, gone.stdout + gone.stderr

    out = subprocess.run([exe, str(tmp_path / "sequences"), "7", "--mask", f"{tmp_path / 'left.png'},{tmp_path / 'right.pgm'}"], cwd=tmp_path, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    traj = np.loadtxt(tmp_path / "07.txt").reshape(-1, 3, 4)
    assert traj.shape[0] == n
    file_prm = lvt_amd.LvtParameters.from_file(str(tmp_path / "vo_config.yaml"))
    orc = O.Oracle(file_prm, 1)
    for i, (L, R) in enumerate(frames):
        Ro, to, _ = MU.oracle_track_masked(orc, file_prm, L, R, ml, mr, f"frame {i}")
        assert orc.status == 2
        _se3_close(traj[i, :, :3], traj[i, :, 3], Ro, to, f"lvt_kitti --mask frame {i}")
    ref = lvt_amd.LvtSystem.create_from_file(str(tmp_path / "vo_config.yaml"), lvt_amd.eSensor_STEREO)
    assert ref.set_mask(ml, mr) == 0, ref.last_error()
    plain = lvt_amd.LvtSystem.create(file_prm, 1)
    differs = False
    for i, (L, R) in enumerate(frames):
        Rm, t = ref.track(L, R)
        Rp, tp = plain.track(L, R)
        differs = differs or not np.array_equal(t, tp)
        assert ref.get_state() == 2 and min(ref.mask_stats()["dropped"]) > 0
        assert np.allclose(traj[i, :, :3], Rm, atol=2e-9) and np.allclose(traj[i, :, 3], t, atol=2e-9), f"frame {i}"
    assert differs, "the masked trajectory is the unmasked one: the comparison shows nothing"

    left_only = subprocess.run([exe, str(tmp_path / "sequences"), "7", "--mask", str(tmp_path / "left.png"), "--out", "left.txt"], cwd=tmp_path, capture_output=True,
                               text=True, timeout=300)
    assert left_only.returncode == 0, left_only.stdout + left_only.stderr
    one = lvt_amd.LvtSystem.create_from_file(str(tmp_path / "vo_config.yaml"), lvt_amd.eSensor_STEREO)
    assert one.set_mask(ml, None) == 0
    t1 = np.loadtxt(tmp_path / "left.txt").reshape(-1, 3, 4)
    for i, (L, R) in enumerate(frames):
        Rm, t = one.track(L, R)
        assert np.allclose(t1[i, :, :3], Rm, atol=2e-9) and np.allclose(t1[i, :, 3], t, atol=2e-9), f"left mask only, frame {i}"


def test_tum_cli_with_a_mask(tmp_path):
    import ctypes as C
    import lvt_amd
    from lvt_amd.synth import make_world
    from oracle import pyoracle as O
    exe = _exe("lvt_tum")
    world = make_world("tum", seed=2, scale=0.5)
    prm = lvt_amd.tum_params(width=world.W, height=world.H, fx=world.fx, fy=world.fy, cx=world.cx, cy=world.cy)
    ds = tmp_path / "root" / "fr1_synth"
    (ds / "rgb").mkdir(parents=True)
    (ds / "depth").mkdir(parents=True)
    (tmp_path / "assoc").mkdir()
    n, frames = 5, []
    with open(tmp_path / "assoc" / "fr1_synth.txt", "w") as af:
        for i in range(n):
            gray, depth = world.render_rgbd(i)
            d16 = np.clip(np.rint(depth.astype(np.float64) * 5000.0), 0, 65535).astype(np.uint16)
            _png(str(ds / "rgb" / f"{i:04d}.png"), gray, filt=(i % 4))
            _png16(str(ds / "depth" / f"{i:04d}.png"), d16)
            af.write(f"{1305031102.175304 + 0.033 * i:.6f} rgb/{i:04d}.png {1305031102.160407 + 0.033 * i:.6f} depth/{i:04d}.png\n")
            frames.append((np.ascontiguousarray(gray), d16.astype(np.float32) * np.float32(1.0 / 5000.0)))
    prm.write_yaml(str(tmp_path / "config.yaml"))
    mask = MU.checkerboard(world.W, world.H)
    _png(str(tmp_path / "mask.png"), mask, filt=1)
    _pgm(str(tmp_path / "wide.pgm"), np.hstack([mask, mask[:, :1]]))
    args = [exe, str(tmp_path / "root"), str(tmp_path / "assoc"), "fr1_synth", str(tmp_path / "config.yaml")]
    bad = subprocess.run(args + ["--mask", str(tmp_path / "wide.pgm"), "--out", "bad.txt"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "wide.pgm is" in bad.stdout and not (tmp_path / "bad.txt").exists(), bad.stdout + bad.stderr
    out = subprocess.run(args + ["--mask", str(tmp_path / "mask.png")], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    traj = np.loadtxt(tmp_path / "fr1_synth.txt").reshape(-1, 8)
    assert traj.shape[0] == n
    file_prm = lvt_amd.LvtParameters.from_file(str(tmp_path / "config.yaml"))
    orc = O.Oracle(file_prm, 2)
    for i, (gray, depth) in enumerate(frames):
        MU.dropped_share(O.detect_grid(gray, file_prm)[0], mask, f"frame {i}", 0.10)
        Ro, to = orc.track_rgbd(gray, MU.masked_depth(depth, mask))
        assert orc.status == 2
        _se3_close(_quat_xyzw_to_R(traj[i, 4:8]), traj[i, 1:4], Ro, to, f"lvt_tum --mask frame {i}")
    L = lvt_amd.load_library()
    pod = lvt_amd.ParamsPOD()
    assert L.lvt_amd_params_from_file(str(tmp_path / "config.yaml").encode(), C.byref(pod)) == 1
    ref = lvt_amd.LvtSystem(L.lvt_amd_create(C.byref(pod), 2), 2)
    assert ref.set_mask(mask) == 0, ref.last_error()
    for i, (gray, depth) in enumerate(frames):
        ref.track(gray, depth)
        assert ref.get_state() == 2
        q, p = ref.pose()
        assert np.allclose(traj[i, 1:4], p, atol=2e-7) and np.allclose(traj[i, 4:8], [q[1], q[2], q[3], q[0]], atol=2e-7), f"frame {i}"
