"""FRAME REDUCTION, the CPU tier: the numpy restatement (reduce_util) against hand-checked answers, lvt_amd_lens_reduced (host code, no device) against the
lens models' forward formulas, and the oracle on the reduced worlds the GPU tier uses -- TRACKING on every frame, with the match counts they were chosen for."""
import numpy as np
import pytest

import lens_util as LU
import reduce_util as RU


def test_hand_checked_answers():
    r = lambda rows, f: int(RU.reduce(np.array(rows, np.uint8), f)[0, 0])
    assert r([[0, 0], [0, 1]], 2) == 0            # S = 1: (1 + 2) // 4
    assert r([[0, 1], [1, 0]], 2) == 1            # S = 2, the tie: (2 + 2) // 4
    assert r([[1, 1, 1], [1, 0, 0], [0, 0, 0]], 3) == 0   # S = 4: (4 + 4) // 9
    assert r([[1, 1, 1], [1, 1, 0], [0, 0, 0]], 3) == 1   # S = 5: (5 + 4) // 9
    assert r(np.full((3, 3), 255), 3) == 255
    assert r(np.full((8, 8), 255), 8) == 255


def test_trailing_columns_and_rows_are_ignored():
    g = np.zeros((7, 8), np.uint8)                # f = 3: 2 x 2 blocks, one trailing row, two trailing columns
    g[6, :] = 255
    g[:, 6:] = 255
    g[0, 0] = 9
    out = RU.reduce(g, 3)
    assert out.shape == (2, 2) and out.tolist() == [[1, 0], [0, 0]]


@pytest.mark.parametrize("f", range(2, 9))
def test_every_sum_image_holds_every_sum(f):
    img = RU.every_sum_image(f)
    S = img.astype(np.uint32).reshape(img.shape[0] // f, f, img.shape[1] // f, f).sum(axis=(1, 3)).reshape(-1)
    assert set(S.tolist()) == set(range(255 * f * f + 1))
    if f == 8:
        assert img.shape == (1024, 1024)
    want = (S * 2 + f * f) // (2 * f * f)         # round half up, computed another way
    if (f * f) % 2 == 1:                          # (odd f f: no ties, (S + (ff >> 1)) / ff is round to nearest)
        want = np.rint(S / (f * f)).astype(np.uint32)
    assert np.array_equal(RU.reduce(img, f).reshape(-1), want.astype(np.uint8))


@pytest.mark.parametrize("model", [LU.RADTAN, LU.FISHEYE], ids=["radtan", "fisheye"])
@pytest.mark.parametrize("f", range(1, 9))
def test_lens_reduced_against_numpy(model, f):
    """a point the full lens projects to (u, v) is projected by the reduced lens to ((u + .5) / f - .5, (v + .5) / f - .5), within 1e-9 px"""
    import lvt_amd
    K = [[1731.3, 0, 1237.9], [0, 1729.8, 611.2], [0, 0, 1]]
    D = [-0.28, 0.07, 2e-4, -3e-4, 0.01, 0.02, -0.01, 0.003, 1e-4, 2e-4, -1e-4, 3e-4] if model == LU.RADTAN else [-0.02, 0.01, -0.004, 0.001]
    full = lvt_amd.Lens(model, 2483, 1235, K, D)
    red = full.reduced(f)
    assert (red.model, red.width, red.height) == (model, 2483 // f, 1235 // f)
    assert np.array_equal(red.D, full.D)
    fx, fy, cx, cy = RU.reduced_intrinsics(K[0][0], K[1][1], K[0][2], K[1][2], f)
    assert np.allclose([red.K[0, 0], red.K[1, 1], red.K[0, 2], red.K[1, 2]], [fx, fy, cx, cy], rtol=0, atol=1e-12)
    assert np.allclose(lvt_amd.reduced_intrinsics(K[0][0], K[1][1], K[0][2], K[1][2], f), [fx, fy, cx, cy], rtol=0, atol=1e-12)
    worst = 0.0
    for x, y in np.random.default_rng(f).uniform(-0.6, 0.6, size=(200, 2)):
        u, v = LU.project(model, full.K, full.D, x, y)
        ur, vr = LU.project(model, red.K, red.D, x, y)
        worst = max(worst, abs(ur - ((u + 0.5) / f - 0.5)), abs(vr - ((v + 0.5) / f - 0.5)))
    print("worst", worst)
    assert worst <= 1e-9


def test_lens_reduced_refusals():
    import lvt_amd
    lens = lvt_amd.Lens(LU.RADTAN, 7, 5, np.eye(3), [])
    for f in (0, -1, 9, 6, 8):                    # (6, 8: a side would reduce to zero)
        with pytest.raises(ValueError):
            lens.reduced(f)
    assert lens.reduced(5).height == 1


WORLDS = [("kitti", (1240, 376), 2, (620, 188), (157, 191)), ("kitti", (1241, 376), 3, (413, 125), (78, 97)),
          ("tum", (640, 480), 2, (320, 240), None), ("tum", (640, 480), 3, (213, 160), None)]


@pytest.mark.parametrize("kind,size,f,small,matches", WORLDS, ids=[f"{w[0]}-f{w[2]}" for w in WORLDS])
def test_oracle_tracks_the_reduced_worlds(oracle_lib, kind, size, f, small, matches):
    q = RU.large_world(kind, 3, size, f)
    assert (q.W, q.H) == small
    orc = q.oracle()
    got = []
    for i in range(6):
        if q.sensor == 1:
            orc.track(*q.small[i])
        else:
            orc.track_rgbd(q.small[i], _registered(q, i))
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        got.append(orc.counts()["n_matches"])
    print("matches", got)
    if matches:
        assert all(matches[0] <= m <= matches[1] for m in got[1:]), got


def _registered(q, i):
    """the depth plane of the large image on the reduced grid, as the tracker's registration makes it: depth_reg_util with identity extrinsics"""
    import depth_reg_util as DR
    return rgbd_depth_on_reduced_grid(DR, q, i)


def rgbd_depth_on_reduced_grid(DR, q, i):
    cam = full_size_depth_camera(q)
    return DR.register(cam, q.prm, q.depth[i])


def full_size_depth_camera(q):
    import lvt_amd
    w = q.world
    return lvt_amd.DepthCamera(width=q.fW, height=q.fH, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy, R=np.eye(3), t=np.zeros(3))
