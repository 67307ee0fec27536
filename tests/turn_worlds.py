"""Two worlds whose camera turns past 180 degrees.  lvt_amd/synth.py turns by at most 4 degrees, so the pose quaternion of every other sequence of the
suite stays at w > 0.99: the w >= 0 flip of the published pose, motion_predict's d < 0 arm, a map point behind the camera and a rotation matrix away from
the identity are reached by nothing else.  Nothing here needs a GPU; the cases built from these worlds are TURN_CASES (case_tables.py).

RolledWorld  a SynthWorld whose camera also rolls about its optical axis by a fixed step per frame.  The layers stay in front of the camera, so the planar
             renderer of the wrapped world draws it: only pose() changes.
RoomWorld    a ray-cast square room.  The camera drives a circle inside it, heading along the tangent: a yaw of a full turn and more, with the walls it has
             passed -- and the map points on them -- behind it.
Both keep their rendered frames (several cases run one world) and are deterministic functions of their seed."""
import copy
import math

import numpy as np

from lvt_amd.synth import SynthWorld


def _rz(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _ry(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


class _Kept:
    """render_stereo / render_rgbd with the frames kept (parity_util._FrameCache's idea); a subclass draws one eye in _render(i, eye, want_depth)"""

    def _init_cache(self):
        self._st, self._rgbd = {}, {}

    def render_stereo(self, i):
        if i not in self._st:
            self._st[i] = (self._render(i, 0, False), self._render(i, 1, False))
        return self._st[i]

    def render_rgbd(self, i):
        if i not in self._rgbd:
            self._rgbd[i] = self._render(i, 0, True)
        return self._rgbd[i]


class RolledWorld(_Kept):
    """`world` with Rz(i * deg_per_frame) applied on the right of its pose: a roll about the optical axis on top of the world's own motion"""

    def __init__(self, world, deg_per_frame):
        self.step = math.radians(deg_per_frame)
        self.W, self.H = world.W, world.H
        self.fx, self.fy, self.cx, self.cy, self.baseline = world.fx, world.fy, world.cx, world.cy, world.baseline
        self._base_pose = world.pose
        self.w = copy.copy(world)       # (shares the layers) the world's own renderer asks ITS pose(): the copy's is the rolled one, `world` stays as it was
        self.w.pose = self.pose
        self._init_cache()

    def pose(self, i):
        R, t = self._base_pose(i)
        return R @ _rz(i * self.step), t

    def _render(self, i, eye, want_depth):
        return self.w.render(i, eye, want_depth)


class RoomWorld(_Kept):
    """a square room of four vertical textured walls at x = +-half_side and z = +-half_side (camera frame convention: x right, y down, z forward).
    Per pixel the ray is R ((u - cx) / fx, (v - cy) / fy, 1); it hits the nearest wall with t > 0 whose along-wall coordinate lies within the room; the
    texel is floor(coordinate / texel) (nearest-texel sampling, no noise).  The ray's camera-frame z is 1, so t IS the planar depth render_rgbd returns.
    pose(i): yaw psi = i * step about y, position radius (1 - cos psi, 0.1 sin(i / 7), sin psi): a circle through the origin whose tangent is the heading."""

    HALF_HEIGHT = 12.0      # metres of wall above and below y = 0 (rows beyond are clamped: no half-size KITTI or TUM ray reaches them)

    def __init__(self, W, H, fx, fy, cx, cy, baseline, half_side=10.0, texel=0.02, seed=0, deg_per_frame=2.5, radius=3.0):
        self.W, self.H = int(W), int(H)
        self.fx, self.fy, self.cx, self.cy, self.baseline = float(fx), float(fy), float(cx), float(cy), float(baseline)
        self.half, self.texel, self.seed = float(half_side), float(texel), int(seed)
        self.step, self.radius = math.radians(deg_per_frame), float(radius)
        rng = np.random.Generator(np.random.PCG64([0x524F4F4D, self.seed]))
        tw, th = int(round(2 * self.half / self.texel)), int(round(2 * self.HALF_HEIGHT / self.texel))
        self.walls = [SynthWorld._make_texture(rng, tw, th, 4000) for _ in range(4)]      # +x, -x, +z, -z
        self._dirs = np.stack([(np.arange(self.W, dtype=np.float64)[None, :] - self.cx) / self.fx + np.zeros((self.H, 1)),
                               (np.arange(self.H, dtype=np.float64)[:, None] - self.cy) / self.fy + np.zeros((1, self.W)),
                               np.ones((self.H, self.W))], axis=-1)
        self._init_cache()

    def pose(self, i):
        psi = i * self.step
        t = self.radius * np.array([1.0 - math.cos(psi), 0.1 * math.sin(i / 7.0), math.sin(psi)])
        return _ry(psi), t

    def _render(self, i, eye, want_depth):
        R, t = self.pose(i)
        c = t + R @ np.array([self.baseline * eye, 0.0, 0.0])
        d = self._dirs @ R.T                                  # (H, W, 3) world-frame rays
        best_t = np.full((self.H, self.W), np.inf)
        img = np.zeros((self.H, self.W), np.uint8)
        th, tw = self.walls[0].shape
        for k, (axis, sign) in enumerate(((0, 1.0), (0, -1.0), (2, 1.0), (2, -1.0))):
            other = 2 - axis
            with np.errstate(divide="ignore", invalid="ignore"):
                tt = (sign * self.half - c[axis]) / d[..., axis]
            along = c[other] + tt * d[..., other]
            with np.errstate(invalid="ignore"):
                hit = (tt > 0) & (np.abs(along) <= self.half) & (tt < best_t)
            a = np.where(hit, along, 0.0)
            y = np.where(hit, c[1] + tt * d[..., 1], 0.0)
            col = np.clip(np.floor((a + self.half) / self.texel), 0, tw - 1).astype(np.int64)
            row = np.clip(np.floor((y + self.HALF_HEIGHT) / self.texel), 0, th - 1).astype(np.int64)
            img = np.where(hit, self.walls[k][row, col], img)
            best_t = np.where(hit, tt, best_t)
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if want_depth:
            return img, np.where(np.isfinite(best_t), best_t, 0.0).astype(np.float32)
        return img
