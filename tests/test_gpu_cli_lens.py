"""examples/lvt_euroc --lens FILE: the calibration of both eyes, the new camera matrix and the tracked size come from a flat key: number file, so a folder
of the mav0 layout with fisheye lenses and raw images of another size than the tracked one runs.  The trajectory is held to the Python route on the same
frames (Rectifier.from_lens, set_rectifiers, LvtSystem.track; numpy for T_BS and the quaternion), and to the oracle fed numpy's remap of the library's maps.
Without the option the program does what tests/test_gpu_cli.py expects of it: that test stays as it is, and a run without --lens is repeated here on a
folder the hard-coded calibration can read."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lens_cases import get_case, N_FRAMES
from parity_util import pose_errors, POSE_TOL
from remap_util import remap
from test_gpu_cli import _png, _quat_xyzw_to_R, _se3_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "lvt_euroc")
def _file_R(q_xyzw):
    """the rotation of a trajectory line.  The file holds the quaternion to 7 digits, so its norm is off by up to ~1e-7, and pose_errors reads the angle from
    arccos of a trace: a trace short by 6e-8 reads as 3.5e-4 rad.  Normalised first, the matrix is a rotation and the angle is the quaternion's own error"""
    q = np.asarray(q_xyzw, np.float64)
    return _quat_xyzw_to_R(q / np.linalg.norm(q))


TBS = np.array([[0.0, -1.0, 0.0, 0.02], [1.0, 0.0, 0.0, -0.06], [0.0, 0.0, 1.0, 0.01]])


def _folder(tmp_path, frames, name="room_synth"):
    ds = tmp_path / "root" / name / "mav0"
    (ds / "cam0" / "data").mkdir(parents=True)
    (ds / "cam1" / "data").mkdir(parents=True)
    (tmp_path / "stamps").mkdir()
    with open(tmp_path / "stamps" / f"{name}.txt", "w") as f:
        for i, (L, R) in enumerate(frames):
            stamp = 1520530308199447626 + 50000000 * i
            _png(str(ds / "cam0" / "data" / f"{stamp}.png"), L, filt=i % 4)
            _png(str(ds / "cam1" / "data" / f"{stamp}.png"), R, filt=(i + 2) % 4)
            f.write(f"{stamp}\n")


def _lens_file(path, c, tbs):
    with open(path, "w") as f:
        f.write("%YAML:1.0\n# a synthetic rig: one equidistant lens for both eyes\n")
        f.write(f"dst_width: {c.dw}\ndst_height: {c.dh}\nbaseline: {float(c.prm.baseline)!r}\n")
        for k, v in enumerate(c.P):
            f.write(f"P{k}: {v!r}\n")
        for eye in ("left", "right"):
            f.write(f"{eye}_model: {c.model}   # fisheye\n{eye}_width: {c.sw}\n{eye}_height: {c.sh}\n")
            for k, v in enumerate(c.K):
                f.write(f"{eye}_K{k}: {v!r}\n")
            for k, v in enumerate(c.D):
                f.write(f"{eye}_D{k}: {v!r}\n")
            for k, v in enumerate(c.R):
                f.write(f"{eye}_R{k}: {v!r}\n")
        if tbs is not None:
            for k, v in enumerate(tbs.reshape(-1)):
                f.write(f"Tbs{k}: {float(v)!r}\n")


@pytest.mark.parametrize("with_tbs", [True, False])
def test_euroc_cli_with_a_lens_file(tmp_path, hip_lib, oracle_lib, with_tbs):
    """a fisheye rig whose raw images (828 x 250) are larger than the tracked size (621 x 187)"""
    import lvt_amd
    c = get_case("fisheye_strong")
    n = 4
    frames = c.raw[:n]
    _folder(tmp_path, frames)
    c.prm.write_yaml(str(tmp_path / "config.yaml"))
    _lens_file(str(tmp_path / "lens.yaml"), c, TBS if with_tbs else None)
    out = subprocess.run([EXE, str(tmp_path / "root"), str(tmp_path / "stamps"), "room_synth", str(tmp_path / "config.yaml"), "--lens", str(tmp_path / "lens.yaml")],
                         cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    traj = np.loadtxt(tmp_path / "room_synth.txt").reshape(-1, 8)
    assert traj.shape[0] == n

    T = np.eye(4)
    if with_tbs:
        T[:3] = TBS
    # the Python route: the parameters as the program derives them (the config's floats; P, the baseline and the size from the lens file, narrowed to float)
    Lib = lvt_amd.load_library()
    pod = lvt_amd.ParamsPOD()
    assert Lib.lvt_amd_params_from_file(str(tmp_path / "config.yaml").encode(), C.byref(pod)) == 1
    pod.fx, pod.fy, pod.cx, pod.cy, pod.baseline = c.P[0], c.P[4], c.P[2], c.P[5], c.prm.baseline
    pod.img_width, pod.img_height = c.dw, c.dh
    ref = lvt_amd.LvtSystem(Lib.lvt_amd_create(C.byref(pod), 1), 1)
    r = c.rectifier(hip_lib)
    assert ref.set_rectifiers(r, r) == 0, ref.last_error()
    oprm = lvt_amd.LvtParameters.from_file(str(tmp_path / "config.yaml"))
    oprm.fx, oprm.fy, oprm.cx, oprm.cy = (float(np.float32(c.P[k])) for k in (0, 4, 2, 5))
    oprm.baseline = float(np.float32(c.prm.baseline))
    oprm.img_width, oprm.img_height = c.dw, c.dh
    orc = oracle_lib.Oracle(oprm, 1)
    m1, m2 = r.maps()
    for i, (Lm, Rm) in enumerate(frames):
        Ro, to = orc.track(remap(Lm, m1, m2)[0], remap(Rm, m1, m2)[0])
        assert orc.status == 2
        To = np.eye(4); To[:3, :3] = Ro; To[:3, 3] = to
        Bo = T @ To
        _se3_close(_file_R(traj[i, 4:8]), traj[i, 1:4], Bo[:3, :3], Bo[:3, 3], f"lvt_euroc --lens frame {i}")
        Rm_, t_ = ref.track(Lm, Rm)
        assert ref.get_state() == 2 and ref.last_error() == "", ref.last_error()
        Tp = np.eye(4); Tp[:3, :3] = Rm_; Tp[:3, 3] = t_
        Bp = T @ Tp
        assert np.allclose(traj[i, 1:4], Bp[:3, 3], atol=2e-6), f"frame {i}: position {traj[i, 1:4]} binding {Bp[:3, 3]}"
        e_t, e_R = pose_errors(_file_R(traj[i, 4:8]), traj[i, 1:4], Bp[:3, :3], Bp[:3, 3])
        assert e_t <= 2e-6 and e_R <= 2e-6, f"frame {i}: e_t {e_t:.2e} e_R {e_R:.2e} against the binding"


def test_euroc_cli_refuses_a_bad_lens_file(tmp_path, hip_lib):
    """a lens file whose two raw sizes differ, and one with an unknown model: the program says why and tracks nothing"""
    c = get_case("fisheye_strong")
    _folder(tmp_path, c.raw[:1])
    c.prm.write_yaml(str(tmp_path / "config.yaml"))
    _lens_file(str(tmp_path / "lens.yaml"), c, None)
    text = open(tmp_path / "lens.yaml").read()
    for bad, word in ((text.replace(f"right_width: {c.sw}", "right_width: 500"), "828 x 250"), (text.replace("left_model: 1", "left_model: 7"), "unknown lens model 7")):
        with open(tmp_path / "bad.yaml", "w") as f:
            f.write(bad)
        out = subprocess.run([EXE, str(tmp_path / "root"), str(tmp_path / "stamps"), "room_synth", str(tmp_path / "config.yaml"), "--lens", str(tmp_path / "bad.yaml")],
                             cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and word in out.stdout, out.stdout + out.stderr
    out = subprocess.run([EXE, str(tmp_path / "root"), str(tmp_path / "stamps"), "room_synth", str(tmp_path / "config.yaml"), "--lens", str(tmp_path / "none.yaml")],
                         cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "lens file" in out.stdout


def test_euroc_cli_without_the_option_is_unchanged(tmp_path, hip_lib):
    """no --lens: the hard-coded EuRoC calibration, 752 x 480 raw images, the trajectory of the Python route with lvt_amd_rectifier_create's rectifiers (two
    frames; tests/test_gpu_cli.py holds the full comparison)"""
    import lvt_amd
    from lvt_amd.synth import make_world
    from test_oracle_primitives import EUROC_L
    CAM1 = dict(K=[457.587, 0.0, 379.999, 0.0, 456.134, 255.238, 0.0, 0.0, 1.0], D=[-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0],
                R=[0.9999633526194376, -0.003625811871560086, 0.007755443660172947, 0.003680398547259526, 0.9999684752771629, -0.007035845251224894,
                   -0.007729688520722713, 0.007064130529506649, 0.999945173484644])
    world = make_world("euroc", seed=1)
    frames = [world.render_stereo(i) for i in range(2)]
    _folder(tmp_path, frames, "MH_synth")
    lvt_amd.euroc_params().write_yaml(str(tmp_path / "config.yaml"))
    out = subprocess.run([EXE, str(tmp_path / "root"), str(tmp_path / "stamps"), "MH_synth", str(tmp_path / "config.yaml")], cwd=tmp_path, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    traj = np.loadtxt(tmp_path / "MH_synth.txt").reshape(-1, 8)
    Lib = lvt_amd.load_library()
    pod = lvt_amd.ParamsPOD()
    assert Lib.lvt_amd_params_from_file(str(tmp_path / "config.yaml").encode(), C.byref(pod)) == 1
    pod.fx = pod.fy = 435.2046959714599
    pod.cx, pod.cy, pod.baseline = 367.4517211914062, 252.2008514404297, 0.110077842
    pod.img_width, pod.img_height = 752, 480
    ref = lvt_amd.LvtSystem(Lib.lvt_amd_create(C.byref(pod), 1), 1)
    rl = lvt_amd.Rectifier(EUROC_L["K"], EUROC_L["D"], EUROC_L["R"], EUROC_L["P"], 752, 480)
    rr = lvt_amd.Rectifier(CAM1["K"], CAM1["D"], CAM1["R"], EUROC_L["P"], 752, 480)
    assert ref.set_rectifiers(rl, rr) == 0
    Tbs = np.array([[0.0148655429818, -0.999880929698, 0.00414029679422, -0.0216401454975], [0.999557249008, 0.0149672133247, 0.025715529948, -0.064676986768],
                    [-0.0257744366974, 0.00375618835797, 0.999660727178, 0.00981073058949], [0, 0, 0, 1.0]])
    for i, (Lm, Rm) in enumerate(frames):
        R, t = ref.track(Lm, Rm)
        Tp = np.eye(4); Tp[:3, :3] = R; Tp[:3, 3] = t
        Bp = Tbs @ Tp
        e_t, e_R = pose_errors(_file_R(traj[i, 4:8]), traj[i, 1:4], Bp[:3, :3], Bp[:3, 3])
        assert e_t <= 2e-6 and e_R <= 2e-6, f"frame {i}: e_t {e_t:.2e} e_R {e_R:.2e} against the binding"
