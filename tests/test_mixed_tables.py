"""The work tables of a mixed lock-step batch (lvt_amd_batch_mixed_tables: host code, no GPU): every (sequence, eye, cell) and every tile of every
image exactly once, cells by non-increasing area over all sequences, tile offsets = prefix sums of the images' tile counts, and each image's tiles
placed over the 8 XCDs in bands of its row-major order.  For the parameter lists tests/test_gpu_mixed_batch.py tracks."""
import numpy as np
import pytest

import lvt_amd

TS_W, TS_H = 64, 16   # k_score's tile (k_features.hip); checked against the table below: the tile rows / columns found must cover the image exactly


def kitti_00_07():
    """KITTI odometry 00 - 07: three calibrations, three image sizes (the reference's examples/kitti/calib)"""
    a = dict(width=1241, height=376, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)
    b = dict(width=1242, height=375, fx=721.5377, fy=721.5377, cx=609.5593, cy=172.854)
    c = dict(width=1226, height=370, fx=707.0912, fy=707.0912, cx=601.8873, cy=183.1104)
    return [lvt_amd.kitti_params(**k) for k in (a, a, a, b, c, c, c, c)]


def everything_different():
    def kitti(w, h, **over):
        p = lvt_amd.kitti_params(width=w, height=h)
        for k, v in over.items():
            setattr(p, k, v)
        return p
    return [kitti(1241, 376, detection_cell_size=257), kitti(1241, 376), kitti(1241, 376, detection_cell_size=100, max_keypoints_per_cell=40),
            kitti(620, 188, tracking_radius=75), kitti(1280, 720), lvt_amd.euroc_params()]


def grid(p):
    cs = p.detection_cell_size
    cx, cy = 1 + (p.img_width - 1) // cs, 1 + (p.img_height - 1) // cs
    return cs, cx, cy


@pytest.mark.parametrize("make", [kitti_00_07, everything_different], ids=["kitti_00_07", "everything_different"])
def test_tables_cover_every_cell_and_tile_once(make):
    prms = make()
    got = lvt_amd.mixed_tables(prms, 1)
    assert got is not None
    cells, score = got
    # ---- cells
    want = {(s, e, c) for s, p in enumerate(prms) for e in (0, 1) for c in range(grid(p)[1] * grid(p)[2])}
    seen = [(int(v >> 16), int((v >> 8) & 0xFF), int(v & 0xFF)) for v in cells]
    assert len(seen) == len(want) and set(seen) == want

    def area(s, c):
        p = prms[s]
        cs, cx, _ = grid(p)
        return min(cs, p.img_width - (c % cx) * cs) * min(cs, p.img_height - (c // cx) * cs)
    areas = [area(s, c) for s, _, c in seen]
    assert all(a >= b for a, b in zip(areas, areas[1:])), "cells are not in non-increasing area order"
    # ---- score tiles: image i owns the workgroups [off_i, off_i + tiles_i), off = prefix sum in image order
    img = (score >> 22).astype(np.int64); by = ((score >> 8) & 0x3FFF).astype(np.int64); bx = (score & 0xFF).astype(np.int64)
    off = 0
    for s, p in enumerate(prms):
        tx, ty = -(-p.img_width // TS_W), -(-p.img_height // TS_H)
        for e in (0, 1):
            n = tx * ty
            sl = slice(off, off + n)
            assert (img[sl] == 2 * s + e).all(), f"image {2 * s + e}: its workgroups are not [{off}, {off + n})"
            t = by[sl] * tx + bx[sl]
            assert (bx[sl] < tx).all() and (by[sl] < ty).all() and sorted(t.tolist()) == list(range(n)), f"image {2 * s + e}: tiles not covered exactly once"
            # workgroup g runs on XCD g & 7: each XCD's tiles are one contiguous run of the row-major order, the runs in XCD order
            g = np.arange(off, off + n)
            lo = 0
            for x in range(8):
                mine = np.sort(t[(g & 7) == x])
                assert mine.tolist() == list(range(lo, lo + len(mine))), f"image {2 * s + e}: XCD {x} does not hold one band of tiles"
                lo += len(mine)
            off += n
    assert off == len(score)


def test_a_multiple_of_eight_reproduces_the_uniform_remap():
    """an image whose workgroups start at a multiple of 8 and whose tile count is one gets what k_score's own formula gives a uniform batch"""
    p = lvt_amd.kitti_params()                     # 20 x 24 = 480 tiles
    _, score = lvt_amd.mixed_tables([p, p], 1)
    n, tx = 480, 20
    for i in range(4):
        for lid in range(n):
            v = int(score[i * n + lid])
            t = (lid & 7) * (n >> 3) + (lid >> 3)
            assert (v >> 22, (v >> 8) & 0x3FFF, v & 0xFF) == (i, t // tx, t % tx)


def test_refused_parameters():
    ok = lvt_amd.kitti_params()
    bad = lvt_amd.kitti_params(width=1241, height=420)
    bad.detection_cell_size = 100                  # 13 x 5 = 65 cells > 64
    assert lvt_amd.mixed_tables([ok, bad], 1) is None
    assert lvt_amd.mixed_tables([ok], 3) is None   # no such sensor type
    tum = lvt_amd.tum_params()
    rgbd = lvt_amd.mixed_tables([tum], 2)          # RGB-D: one image per sequence
    assert rgbd is not None and len(rgbd[0]) == grid(tum)[1] * grid(tum)[2] and set((rgbd[1] >> 22).tolist()) == {0}
