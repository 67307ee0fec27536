"""Unregistered depth (lvt_amd_set_depth_camera): the numpy restatement of the registration -- include/lvt_amd_ext.h, UNREGISTERED DEPTH, operation for
operation in fp32 --, the depth-camera renderer of the synthetic worlds and the sequences the CPU and GPU tests share."""
import copy

import numpy as np

import lvt_amd
from parity_util import make_case
from rgbd_util import SCALE, quantise

F = np.float32
MAX_SPAN = 16
INF_BITS = np.uint32(0x7F800000)


def make_camera(width, height, fx, fy, cx, cy, R=None, t=None):
    return lvt_amd.DepthCamera(width, height, fx, fy, cx, cy, R, t)


def identity_camera(prm):
    """the colour camera itself: K_d = K_c, R = I, t = 0, the image's size (with an undistorted colour camera every footprint is its own pixel)"""
    return make_camera(prm.img_width, prm.img_height, prm.fx, prm.fy, prm.cx, prm.cy)


def rot(axis, deg):
    a = np.radians(deg); c, s = np.cos(a), np.sin(a)
    return {0: np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), 1: np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), 2: np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def register_numpy(cam, prm, depth, depth_scale=None, pitch=None, counts=None):
    """(the registered plane, float32 (img_height, pitch or img_width), +inf where nothing landed; the largest footprint (columns, rows)).  depth: float32
    (cam.height, cam.width), or uint16 with depth_scale.  Every operation is one fp32 operation, in the order the header writes them.  counts: an int array of
    img_height * pitch that takes the number of writes every word received."""
    W, H = int(prm.img_width), int(prm.img_height)
    pitch = W if pitch is None else int(pitch)
    dw, dh = int(cam.width), int(cam.height)
    depth = np.asarray(depth)
    assert depth.shape == (dh, dw), (depth.shape, dh, dw)
    if depth.dtype == np.uint16:
        z = depth.astype(F) * F(depth_scale)
    else:
        assert depth.dtype == F
        z = depth
    fxd, fyd, cxd, cyd = F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy)
    Rm, tv = cam.R.astype(F), cam.t.astype(F)
    fx, fy, cx, cy = F(prm.fx), F(prm.fy), F(prm.cx), F(prm.cy)
    k1, k2, p1, p2, k3 = F(prm.k1), F(prm.k2), F(prm.p1), F(prm.p2), F(prm.k3)
    one, two, half = F(1), F(2), F(0.5)
    ci = np.arange(dw, dtype=F)[None, :]
    cj = np.arange(dh, dtype=F)[:, None]

    def proj(a, b):
        X = ((a - cxd) / fxd) * z
        Y = ((b - cyd) / fyd) * z
        Xc = (Rm[0, 0] * X + Rm[0, 1] * Y) + Rm[0, 2] * z + tv[0]
        Yc = (Rm[1, 0] * X + Rm[1, 1] * Y) + Rm[1, 2] * z + tv[1]
        Zc = (Rm[2, 0] * X + Rm[2, 1] * Y) + Rm[2, 2] * z + tv[2]
        x = Xc / Zc
        y = Yc / Zc
        r2 = x * x + y * y
        rad = one + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = x * rad + (two * p1 * x * y + p2 * (r2 + two * x * x))
        yd = y * rad + (p1 * (r2 + two * y * y) + two * p2 * x * y)
        return xd * fx + cx, yd * fy + cy, Zc

    out = np.full(H * pitch, INF_BITS, dtype=np.uint32)
    with np.errstate(all="ignore"):
        u0, v0, _ = proj(ci - half, cj - half)
        u1, v1, _ = proj(ci + half, cj + half)
        _, _, Zc = proj(ci, cj)
        for a in (u0, v0, u1, v1, Zc):
            assert a.dtype == F and a.shape == (dh, dw)
        ok = np.isfinite(z) & (z > 0) & np.isfinite(Zc) & (Zc > 0)
        for a in (u0, v0, u1, v1):
            ok &= np.abs(a) < F(1e6)          # (False for NaN and infinities)
        c = [np.where(ok, np.ceil(a), F(0)).astype(np.int64) for a in (u0, v0, u1, v1)]
    x0, y0, x1, y1 = c[0], c[1], c[2] - 1, c[3] - 1
    ok &= (x1 - x0 < MAX_SPAN) & (y1 - y0 < MAX_SPAN)
    x0, y0, x1, y1 = np.maximum(x0, 0), np.maximum(y0, 0), np.minimum(x1, W - 1), np.minimum(y1, H - 1)
    ok &= (x0 <= x1) & (y0 <= y1)
    zb = np.ascontiguousarray(Zc).view(np.uint32)
    nx = int((x1 - x0)[ok].max()) + 1 if ok.any() else 0
    ny = int((y1 - y0)[ok].max()) + 1 if ok.any() else 0
    assert nx <= MAX_SPAN and ny <= MAX_SPAN
    for dy in range(ny):                       # one pass per footprint offset
        for dx in range(nx):
            m = ok & (x0 + dx <= x1) & (y0 + dy <= y1)
            np.minimum.at(out, ((y0 + dy) * pitch + (x0 + dx))[m], zb[m])
            if counts is not None:
                np.add.at(counts, ((y0 + dy) * pitch + (x0 + dx))[m], 1)
    return out.view(F).reshape(H, pitch), (nx, ny)


def register(cam, prm, depth, depth_scale=None, pitch=None):
    return register_numpy(cam, prm, depth, depth_scale, pitch)[0]


def holes(reg, W):
    return float(np.isinf(reg[:, :W]).mean())


# ---- the depth camera of a synthetic world ---------------------------------------------------------------------------------------------------
def render_depth_camera(world, i, cam):
    """the depth image a second camera sees: a shallow copy of the world whose K, W, H and baseline are the depth camera's, rendered as eye 1 (a world BUILT at
    another size has other textures).  The camera sits at t = (b, 0, 0) of the colour frame, R = I."""
    w = getattr(world, "w", world)             # (parity_util's frame cache wraps the world)
    assert np.array_equal(cam.R, np.eye(3, dtype=F)) and cam.t[1] == 0 and cam.t[2] == 0
    d = copy.copy(w)
    d.W, d.H, d.baseline = int(cam.width), int(cam.height), float(cam.t[0])
    d.K = np.array([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], dtype=np.float64)
    d._torch_cache = None
    return d.render(i, 1, want_depth=True)[1]


def offset_camera(prm, width, height, baseline=0.05, focal=0.9, shift=(1.7, -1.3)):
    """a depth camera `baseline` metres to the side: the colour intrinsics scaled to width x height, focal lengths times `focal`, principal point shifted"""
    sx, sy = width / prm.img_width, height / prm.img_height
    return make_camera(width, height, prm.fx * sx * focal, prm.fy * sy * focal, prm.cx * sx + shift[0] * sx, prm.cy * sy + shift[1] * sy, None, (baseline, 0, 0))


class DSeq:
    """one RGB-D sequence whose depth comes from a depth camera: gray frames; the SENSOR's planes s_u16 (quantised like rgbd_util's) and s_f32 = s_u16 * SCALE;
    f32 = their numpy registration -- what the oracle is fed, under the name rgbd_util's helpers read.  cam None: an ordinary registered sequence."""

    def __init__(self, seed, size, n, cam_of=None, overrides=None):
        self.world, self.prm, sensor = make_case("tum", seed, 1.0, overrides, size)
        assert sensor == 2
        self.W, self.H, self.n = self.world.W, self.world.H, n
        self.cam = cam_of(self.prm) if cam_of else None
        self.gray, self.s_u16, self.s_f32, self.f32, self.holes = [], [], [], [], []
        for i in range(n):
            g, d = self.world.render_rgbd(i)
            if self.cam is not None:
                d = render_depth_camera(self.world, i, self.cam)
            u = quantise(d)
            self.gray.append(np.ascontiguousarray(g)); self.s_u16.append(u); self.s_f32.append(u.astype(F) * SCALE)
            if self.cam is not None:
                self.f32.append(register(self.cam, self.prm, u, SCALE))
                self.holes.append(holes(self.f32[-1], self.W))
            else:
                self.f32.append(self.s_f32[-1])
        self.dw, self.dh = (self.cam.width, self.cam.height) if self.cam is not None else (self.W, self.H)


_SEQS = {}


def sequence(which, n=12):
    """the two 320 x 240 TUM-shaped sequences of the tests ('same', 'half'; 'big': a depth camera LARGER than the image; 'plain': the same world with
    registered depth), built once per process"""
    key = (which, n)
    if key not in _SEQS:
        cam_of = {"same": lambda p: offset_camera(p, 320, 240), "half": lambda p: offset_camera(p, 160, 120), "big": lambda p: offset_camera(p, 400, 300),
                  "plain": None}[which]
        _SEQS[key] = DSeq(0, (320, 240), n, cam_of)
    return _SEQS[key]


# ---- the constructed 8 x 6 case ----------------------------------------------------------------------------------------------------------------
# Colour camera 8 x 6, fx = fy = 1, cx = cy = 0, no distortion; depth camera 8 x 6 with the same pinhole: depth pixel (i, j) at depth z with R = I lands at
# u = (i z + t0) / (z + t2).  With t = 0 a pixel's footprint is exactly itself (corners i -+ 0.5 -> ceil gives [i, i]).
def constructed_case():
    """(cases, prm): each case (cam, depth, expected) with the expected plane written out by hand"""
    prm = lvt_amd.tum_params(width=8, height=6, fx=1.0, fy=1.0, cx=0.0, cy=0.0)
    inf, nan = F(np.inf), F(np.nan)
    cases = {}
    # (a) invalid depths: z = 0, NaN, -1, +inf leave no trace; their neighbours map to themselves
    d = np.full((6, 8), 2.0, F)
    d[1, 1], d[1, 2], d[1, 3], d[1, 4] = 0.0, nan, -1.0, inf
    e = d.copy(); e[1, 1:5] = inf
    cases["invalid depths"] = (make_camera(8, 6, 1, 1, 0, 0), d, e)
    # (b) two depth pixels on one colour pixel, the nearer wins.  Footprints only double up through depth: two pixels of different z and a translation.
    #     t = (2, 0, 0), rows of z = 2 except pixel (5, 3) with z = 1: z = 2 -> u = (2 i + 2) / 2 = i + 1 (footprint column i + 1);
    #     z = 1 -> u = (5 + 2) / 1 = 7: corners (4.5 + 2, 5.5 + 2) = [ceil(6.5), ceil(7.5) - 1] = [7, 7]; rows: v = j for both.  Colour (7, 3) gets z = 2 from depth (6, 3) and
    #     z = 1 from depth (5, 3): 1 wins.  Colour (6, 3) is a hole (its depth pixel (5, 3) went elsewhere); column 0 is a hole in every row; depth column 7 leaves the image.
    d = np.full((6, 8), 2.0, F); d[3, 5] = 1.0
    e = np.full((6, 8), 2.0, F); e[:, 0] = inf; e[3, 6] = inf; e[3, 7] = 1.0
    cases["nearer wins"] = (make_camera(8, 6, 1, 1, 0, 0, None, (2, 0, 0)), d, e)
    # (c) a 180-degree extrinsic about y: Zc = -z <= 0 for every pixel: nothing lands
    cases["behind the camera"] = (make_camera(8, 6, 1, 1, 0, 0, rot(1, 180), None), np.full((6, 8), 2.0, F), np.full((6, 8), inf, F))
    # (d) footprints cut by each image edge and one wholly outside: depth fx_d = fy_d = 0.5, z = 1, t = 0: u = 2 i, corners 2 i -+ 1 -> columns [2 i - 1, 2 i]; rows likewise.
    #     only four pixels carry depth: (0, 0) -> columns [-1, 0], rows [-1, 0]: cut by the left and top edges -> (0, 0);
    #     (4, 3) -> columns [7, 8], rows [5, 6]: cut by the right and bottom edges -> (7, 5); (2, 1) -> columns [3, 4], rows [1, 2] whole; (7, 5) -> columns [13, 14]: outside.
    d = np.zeros((6, 8), F); d[0, 0], d[3, 4], d[1, 2], d[5, 7] = 1.0, 1.5, 2.5, 3.0
    e = np.full((6, 8), inf, F); e[0, 0] = 1.0; e[5, 7] = 1.5; e[1:3, 3:5] = 2.5
    cases["edges"] = (make_camera(8, 6, 0.5, 0.5, 0, 0), d, e)
    return cases, prm


def span_case(diff, axis):
    """one depth pixel whose footprint has x1 - x0 = diff (15: kept, the widest allowed; 16: skipped) along `axis` (0: columns, 1: rows) and is one pixel the
    other way.  Colour 40 x 40 (fx = fy = 1, c = 0); depth pixel (1, 1) of a 4 x 4 depth camera with 1 / f_d = s = diff + 1 along the axis: u = s i, corners
    s / 2 and 3 s / 2 -> [ceil(s / 2), ceil(3 s / 2) - 1].  s = 16: [8, 23] (every value exact); s = 17: corners 8.5 and 25.5 -> [9, 25] (f_d = 1 / 17 is
    rounded, the corners stay far from an integer)."""
    assert diff in (15, 16)
    s = diff + 1
    prm = lvt_amd.tum_params(width=40, height=40, fx=1.0, fy=1.0, cx=0.0, cy=0.0)
    cam = make_camera(4, 4, 1.0 / s if axis == 0 else 1.0, 1.0 / s if axis == 1 else 1.0, 0, 0)
    d = np.zeros((4, 4), F); d[1, 1] = 2.0
    e = np.full((40, 40), np.inf, F)
    if diff < MAX_SPAN:
        if axis == 0:
            e[1, 8:24] = 2.0
        else:
            e[8:24, 1] = 2.0
    return cam, prm, d, e
