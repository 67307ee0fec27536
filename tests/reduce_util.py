"""FRAME REDUCTION in numpy: the definition of include/lvt_amd_ext.h restated, and the large worlds the reduction tests share.  No expected value in the
tests comes from the library under test: frames are reduced HERE and the unchanged oracle is fed the reduced frames with the reduced intrinsics."""
import numpy as np

import lvt_amd
from lvt_amd.synth import make_world


def reduce(g, f):
    """the f x f block mean of a gray image: out[y][x] = (S + f*f // 2) // (f*f), S the block's sum; up to f - 1 trailing columns and rows are ignored"""
    g = np.asarray(g)
    assert g.ndim == 2 and g.dtype == np.uint8 and 2 <= f <= 8
    h, w = g.shape[0] // f, g.shape[1] // f
    S = g[:h * f, :w * f].astype(np.uint32).reshape(h, f, w, f).sum(axis=(1, 3))
    return ((S + (f * f) // 2) // (f * f)).astype(np.uint8)


def reduced_intrinsics(fx, fy, cx, cy, f):
    """reduced pixel x covers source [f x, f x + f): fx' = fx / f, cx' = (cx + 0.5) / f - 0.5 (restated here; lvt_amd.reduced_intrinsics is held to it)"""
    return fx / f, fy / f, (cx + 0.5) / f - 0.5, (cy + 0.5) / f - 0.5


def every_sum_image(f):
    """an image whose f x f blocks take every sum 0 ... 255 f f once (block i has sum i: i // (f f) everywhere, + 1 on i % (f f) scattered pixels), padded
    with zero blocks to a rectangle; at f = 8: 16 321 sums, a 1 024 x 1 024 image"""
    ff = f * f
    n = 255 * ff + 1
    side = int(np.ceil(np.sqrt(n)))
    blocks = np.zeros((side * side, ff), np.uint16)
    i = np.arange(n)
    blocks[:n] = (i // ff)[:, None]
    order = np.random.default_rng(f).permutation(ff)           # which pixels of a block carry the remainder
    blocks[:n] += (np.argsort(order)[None, :] < (i % ff)[:, None]).astype(np.uint16)
    assert blocks.max() == 255 and np.array_equal(blocks[:n].sum(axis=1), i)
    img = blocks.reshape(side, side, f, f).transpose(0, 2, 1, 3).reshape(side * f, side * f).astype(np.uint8)
    return np.ascontiguousarray(img)


class _Frames:
    """frames 0 ... n - 1 of a world, each made when first asked for and kept"""

    def __init__(self, n, make):
        self.n, self.make, self.kept = n, make, {}

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self.n))]
        if not 0 <= i < self.n:
            raise IndexError(i)
        if i not in self.kept:
            self.kept[i] = self.make(i)
        return self.kept[i]


class LargeWorld:
    """a synthetic world rendered at `size`, tracked at size // f: the large frames, their numpy reduction, the parameters of the reduced image"""

    def __init__(self, kind, seed, size, f, n):
        self.kind, self.f, self.n = kind, f, n
        self.world = w = make_world(kind, seed=seed, size=size)
        self.fW, self.fH = w.W, w.H
        self.W, self.H = w.W // f, w.H // f
        self.pitch = (self.W + 63) // 64 * 64
        self.sensor = 2 if kind == "tum" else 1
        fx, fy, cx, cy = reduced_intrinsics(w.fx, w.fy, w.cx, w.cy, f)
        mk = {"kitti": lvt_amd.kitti_params, "tum": lvt_amd.tum_params}[kind]
        kw = dict(width=self.W, height=self.H, fx=fx, fy=fy, cx=cx, cy=cy)
        if kind != "tum":
            kw["baseline"] = w.baseline
        self.prm = mk(**kw)
        # (rendered when first asked for: a full-size frame costs far more CPU than tracking its reduction)
        if self.sensor == 1:
            self.large = _Frames(n, lambda i: tuple(np.ascontiguousarray(a) for a in w.render_stereo(i)))
            self.small = _Frames(n, lambda i: tuple(reduce(a, f) for a in self.large[i]))
        else:
            both = _Frames(n, lambda i: w.render_rgbd(i))
            self.large = _Frames(n, lambda i: np.ascontiguousarray(both[i][0]))
            self.depth = _Frames(n, lambda i: np.ascontiguousarray(both[i][1], dtype=np.float32))
            self.small = _Frames(n, lambda i: reduce(self.large[i], f))
        self._chains = {}

    def reduction(self):
        return lvt_amd.Reduction(self.f, self.fW, self.fH)

    def oracle(self):
        from oracle import pyoracle as O
        return O.Oracle(self.prm, self.sensor)

    def chain(self, frames=None, images=None):
        """[(R, t, state, counts)] of the oracle over `frames` of the reduced stereo images (or of `images`), asserted TRACKING throughout"""
        frames = tuple(range(self.n)) if frames is None else tuple(frames)
        key = (frames, id(images))
        if key not in self._chains:
            orc, out = self.oracle(), []
            for i in frames:
                R, t = orc.track(*(images or self.small)[i])
                out.append((np.array(R), np.array(t), orc.status, orc.counts()))
            assert [r[2] for r in out] == [2] * len(out), "the oracle is not TRACKING on every frame: an early LOST would hide a difference"
            self._chains[key] = out
        return self._chains[key]


_WORLDS = {}


def large_world(kind="kitti", seed=3, size=(1240, 376), f=2, n=40):
    key = (kind, seed, tuple(size), f, n)
    if key not in _WORLDS:
        _WORLDS[key] = LargeWorld(kind, seed, size, f, n)
    return _WORLDS[key]
