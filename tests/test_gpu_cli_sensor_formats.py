"""examples/lvt_kitti --bayer PATTERN and examples/lvt_euroc --mono16 LO,HI | auto[,LOPM,HIPM,SPAN]: the files hold the sensor's samples and the feature stage
converts them.  The trajectory file must be the one the program writes, WITHOUT the option, on the numpy-converted images -- byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import colour_util as CU
import lvt_amd
import sensor_util as SU
from test_gpu_cli import _png
from test_gpu_cli_reduction import _dataset, _run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("pattern", ["RGGB", "GBRG"])
def test_kitti_cli_bayer_equals_the_cli_on_converted_pngs(tmp_path, hip_lib, pattern):
    from parity_util import make_case
    fmt = {"RGGB": SU.RGGB, "GBRG": SU.GBRG}[pattern]
    world, _, _ = make_case("kitti", 71, size=(621, 187))
    n = 5
    raw = [tuple(SU.mosaic(*CU.colour_channels(np.ascontiguousarray(g), 71, i, eye)[:3], fmt) for eye, g in enumerate(world.render_stereo(i))) for i in range(n)]
    conv = [tuple(SU.bayer_to_gray(m, fmt) for m in pair) for pair in raw]
    a, b = tmp_path / "mosaic", tmp_path / "gray"
    a.mkdir(); b.mkdir()
    _dataset(a, raw, world.fx, world.fy, world.cx, world.cy, world.baseline)
    _dataset(b, conv, world.fx, world.fy, world.cx, world.cy, world.baseline)
    for d in (a, b):
        lvt_amd.kitti_params().write_yaml(str(d / "config.yaml"))
    got, want = _run(a, "--bayer", pattern), _run(b)
    assert len(want.splitlines()) == n
    assert got == want
    assert _run(a) != want                      # (the mosaic tracked as if it were gray is another trajectory: the option did something)


def _pgm16(path, img16):
    """binary PGM, maxval 65535: two bytes per sample, most significant first"""
    with open(path, "wb") as f:
        f.write(b"P5\n# sixteen bit\n%d %d\n65535\n" % (img16.shape[1], img16.shape[0]))
        f.write(img16.astype(">u2").tobytes())


@pytest.mark.parametrize("option,rec", [("19990,20790", SU.Record(SU.MONO16, lo=19990, hi=20790)), ("auto,5,5,256", SU.THERMAL), ("auto", SU.THERMAL)],
                         ids=["fixed", "auto", "auto-defaults"])
def test_euroc_cli_mono16_equals_the_cli_on_converted_pngs(tmp_path, hip_lib, option, rec):
    from lvt_amd.synth import make_world
    exe = os.path.join(ROOT, "examples", "lvt_euroc")
    world = make_world("euroc", seed=1)
    n = 4
    for name in ("raw", "gray"):
        for cam in ("cam0", "cam1"):
            (tmp_path / name / "MH_synth" / "mav0" / cam / "data").mkdir(parents=True)
    (tmp_path / "stamps").mkdir()
    with open(tmp_path / "stamps" / "MH_synth.txt", "w") as f:
        for i in range(n):
            stamp = 1403636579763555584 + 50000000 * i
            f.write(f"{stamp}\n")
            for e, g in enumerate(world.render_stereo(i)):
                t16 = SU.thermal(np.ascontiguousarray(g), 2 * i + e)
                _pgm16(str(tmp_path / "raw" / "MH_synth" / "mav0" / f"cam{e}" / "data" / f"{stamp}.pgm"), t16)
                _png(str(tmp_path / "gray" / "MH_synth" / "mav0" / f"cam{e}" / "data" / f"{stamp}.png"), SU.convert(t16, rec)[0], filt=i % 4)
    lvt_amd.euroc_params().write_yaml(str(tmp_path / "config.yaml"))
    outs = []
    for name, extra in (("raw", ["--mono16", option]), ("gray", [])):
        out = subprocess.run([exe, str(tmp_path / name), str(tmp_path / "stamps"), "MH_synth", str(tmp_path / "config.yaml"), "--out", str(tmp_path / (name + ".txt")), *extra],
                             cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        outs.append(open(tmp_path / (name + ".txt"), "rb").read())
    lines = outs[1].splitlines()
    assert len(lines) == n and not lines[1].endswith(b" 0.0000000 0.0000000 0.0000000 0.0000000 0.0000000 0.0000000 1.0000000"), "frame 1 was not tracked: nothing is compared"
    assert outs[0] == outs[1]
