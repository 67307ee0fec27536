"""examples/lvt_tum --depth-guard: the record is parsed and handed to the tracker before the first frame.  The trajectory under 1,6,0.01,0.02 is held FIRST
against the oracle fed the guarded plane (depth_guard_util), then -- tighter, as a plumbing check -- against the Python binding with the same record; the bare
flag is held to the binding under lvt_amd_depth_guard_default's record.  A record outside its ranges, or one that does not parse, is refused with a message and
a non-zero exit before any frame is tracked."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import depth_guard_util as DG
from test_gpu_cli import _png, _png16, _se3_close, _quat_xyzw_to_R
from test_gpu_cli_masks import _exe

pytestmark = pytest.mark.gpu


def test_tum_cli_with_a_depth_guard(tmp_path):
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
    args = [exe, str(tmp_path / "root"), str(tmp_path / "assoc"), "fr1_synth", str(tmp_path / "config.yaml")]

    def run(*more):
        return subprocess.run(args + list(more), cwd=tmp_path, capture_output=True, text=True, timeout=300)

    bad = run("--depth-guard", "1,9,0.01,0.02", "--out", "bad.txt")
    assert bad.returncode != 0 and "min_support = 9 at radius 1 (1 ... 8)" in bad.stdout and not (tmp_path / "bad.txt").exists(), bad.stdout + bad.stderr
    bad = run("--depth-guard", "1,6", "--out", "bad.txt")
    assert bad.returncode != 0 and "R,N,ABS,REL" in bad.stdout and not (tmp_path / "bad.txt").exists(), bad.stdout + bad.stderr

    out = run("--depth-guard", "1,6,0.01,0.02")
    assert out.returncode == 0, out.stdout + out.stderr
    traj = np.loadtxt(tmp_path / "fr1_synth.txt").reshape(-1, 8)
    assert traj.shape[0] == n
    file_prm = lvt_amd.LvtParameters.from_file(str(tmp_path / "config.yaml"))
    near, far = file_prm.near_plane_distance, file_prm.far_plane_distance
    orc = O.Oracle(file_prm, 2)
    for i, (gray, depth) in enumerate(frames):
        DG.dropped_share(O.detect_grid(gray, file_prm)[0], depth, DG.STRICT, near, far, f"frame {i}", 0.05)
        Ro, to = orc.track_rgbd(gray, DG.guarded_depth(depth, DG.STRICT, near, far))
        assert orc.status == 2
        _se3_close(_quat_xyzw_to_R(traj[i, 4:8]), traj[i, 1:4], Ro, to, f"lvt_tum --depth-guard frame {i}")

    L = lvt_amd.load_library()
    pod = lvt_amd.ParamsPOD()
    assert L.lvt_amd_params_from_file(str(tmp_path / "config.yaml").encode(), C.byref(pod)) == 1

    def binding(cfg):
        ref, poses = lvt_amd.LvtSystem(L.lvt_amd_create(C.byref(pod), 2), 2), []
        if cfg is not None:
            assert ref.set_depth_guard(cfg) == 0, ref.last_error()
        for gray, depth in frames:
            ref.track(gray, depth)
            assert ref.get_state() == 2
            q, p = ref.pose()
            poses.append(np.concatenate([p, [q[1], q[2], q[3], q[0]]]))
        return np.array(poses)

    guarded, plain = binding(lvt_amd.DepthGuard(1, 6, 0.01, 0.02)), binding(None)
    assert np.allclose(traj[:, 1:8], guarded, atol=2e-7)
    assert not np.array_equal(guarded, plain), "the guarded trajectory is the unguarded one: the comparison shows nothing"

    out = run("--max-frames", "4", "--depth-guard", "--out", "bare.txt")     # the bare flag in front of another option ...
    assert out.returncode == 0 and "Frames: 4/4" in out.stdout, out.stdout + out.stderr
    out = run("--out", "bare.txt", "--depth-guard")                         # ... and as the last argument
    assert out.returncode == 0, out.stdout + out.stderr
    bare = np.loadtxt(tmp_path / "bare.txt").reshape(-1, 8)
    assert np.allclose(bare[:, 1:8], binding(lvt_amd.depth_guard_default()), atol=2e-7)
