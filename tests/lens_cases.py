"""The tracking worlds of the lens-model tests (tests/test_lens_models.py on the CPU, tests/test_gpu_lens_models.py on the GPU): the kitti world, seed 71,
rendered at a SOURCE size, seen through a lens record whose K is that rendering's intrinsics, and rectified to a DESTINATION size whose P is the intrinsics
the same world has at that size (R = I).  The lens is a warp laid over pinhole frames: what matters is that both eyes go through one map, so the rectified
pair stays row-aligned and the tracker has work it can do.

  fisheye_strong  FISHEYE D = [0.6, 0.05, 0, 0], 828 x 250 -> 621 x 187: 12.0 % of the map entries fall outside the source (the border branches run)
  fisheye_mild    FISHEYE D = [-0.02, 0.004, -0.001, 0.0002], 828 x 250 -> 621 x 187: none do
  radtan12        RADTAN, twelve coefficients, 817 x 247 -> 613 x 185: 7.4 % do
  fisheye_small   fisheye_strong's lens on a source SMALLER than the destination: 500 x 150 -> 621 x 187
  radtan_small    radtan12's lens likewise (the plane tests only: nothing tracks it)
A case's frames, maps and rectified frames are computed once and shared."""
import numpy as np

from lens_util import RADTAN, FISHEYE, lens_maps
from parity_util import make_case
from remap_util import remap

EYE3 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
RADTAN12 = [0.12, 0.02, 2e-4, -1e-4, 0.01, 0.05, 0.01, 0.002, 1e-3, -5e-4, 5e-4, 1e-3]
SPECS = {
    "fisheye_strong": (FISHEYE, [0.6, 0.05, 0.0, 0.0], (828, 250), (621, 187)),
    "fisheye_mild": (FISHEYE, [-0.02, 0.004, -0.001, 0.0002], (828, 250), (621, 187)),
    "radtan12": (RADTAN, RADTAN12, (817, 247), (613, 185)),
    "fisheye_small": (FISHEYE, [0.6, 0.05, 0.0, 0.0], (500, 150), (621, 187)),
    "radtan_small": (RADTAN, RADTAN12, (500, 150), (621, 187)),
}
N_FRAMES = 8


def world_K(world):
    return [world.fx, 0.0, world.cx, 0.0, world.fy, world.cy, 0.0, 0.0, 1.0]


class LensCase:
    def __init__(self, name):
        self.name = name
        self.model, self.D, (self.sw, self.sh), (self.dw, self.dh) = SPECS[name]
        src_world, _, _ = make_case("kitti", 71, size=(self.sw, self.sh))
        _, self.prm, _ = make_case("kitti", 71, size=(self.dw, self.dh))
        dst_world, _, _ = make_case("kitti", 71, size=(self.dw, self.dh))
        self.K, self.P, self.R = world_K(src_world), world_K(dst_world), EYE3
        self.pitch = ((self.dw + 63) // 64) * 64
        self.raw = [tuple(np.ascontiguousarray(x) for x in src_world.render_stereo(i)) for i in range(N_FRAMES)]
        self._rect = {}

    def numpy_maps(self):
        return lens_maps(self.model, self.K, self.D, self.R, self.P, self.dw, self.dh)

    def rectified(self, maps=None, key="numpy"):
        """the raw frames through remap_util.remap under `maps` (default: the numpy restatement's), [(left, right)]; kept under `key`"""
        if key not in self._rect:
            m1, m2 = self.numpy_maps() if maps is None else maps
            self._rect[key] = [(remap(a, m1, m2)[0], remap(b, m1, m2)[0]) for a, b in self.raw]
        return self._rect[key]

    def lens(self, hip_lib):
        return hip_lib.Lens(self.model, self.sw, self.sh, self.K, self.D)

    def rectifier(self, hip_lib):
        return hip_lib.Rectifier.from_lens(self.lens(hip_lib), self.R, self.P, self.dw, self.dh)


_CASES = {}


def get_case(name):
    if name not in _CASES:
        _CASES[name] = LensCase(name)
    return _CASES[name]
