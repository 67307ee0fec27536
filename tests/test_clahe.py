"""CPU tier of the equalisation (include/lvt_amd_ext.h, DIM frames): tests/clahe_util.py -- the numpy restatement every GPU test compares against -- is held
to answers worked out by hand; lvt_amd_equalisation_plan (host code of the library, no GPU) is held to clahe_util.plan; and the ORACLE alone shows what the
property is for: LOST on a dimmed world, TRACKING on the same frames equalised.  No expected value comes from the library."""
import numpy as np
import pytest

import clahe_util as CL
from parity_util import make_case

SIZES = [((64, 64), (8, 8)), ((70, 50), (8, 8)), ((65, 33), (8, 4)), ((97, 83), (16, 16)), ((67, 64), (4, 2)), ((1241, 376), (8, 8))]
CLIPS = [0.01, 1.0, 3.0, 40.0, 1e9]


# ---- the util against hand-checked answers ---------------------------------------------------------------------------------------------------
def test_a_uniform_tile_without_clipping():
    """one 16 x 16 tile that holds every level once, a clip limit that does not clip: hist = 1 everywhere, cum[i] = i + 1, lut[i] = rint((i + 1) 255 / 256)"""
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    p = CL.plan(16, 16, (1, 1), 1e9)
    assert (p["area"], p["clip"]) == (256, 256)
    L = CL.luts(img, (1, 1), 1e9)
    want = np.rint((np.arange(256) + 1) * 255.0 / 256.0).astype(np.uint8)    # (exact in fp64 and in fp32: 255 / 256 is a binary fraction)
    assert np.array_equal(L[0, 0], want)
    assert L[0, 0, 0] == 1 and L[0, 0, 255] == 255
    assert L[0, 0, 127] == 128 and L[0, 0, 126] == 127     # 128 * 255 / 256 = 127.5, the one tie: half to even gives 128; 127 * 255 / 256 = 126.50390625


def test_a_constant_image():
    """32 x 32, one tile, every pixel 77, clip limit 2: area 1024, clip = (int)(2 * 1024 / 256) = 8, excess 1016 = 3 * 256 + 248, step = max(256 / 248, 1) = 1:
    bins 0 ... 247 hold 4, bins 248 ... 255 hold 3, bin 77 holds 8 + 4 = 12.  cum[77] = 77 * 4 + 12 = 320, lut[77] = rint(320 * 255 / 1024) = rint(79.6875) = 80"""
    img = np.full((32, 32), 77, np.uint8)
    assert CL.plan(32, 32, (1, 1), 2.0)["clip"] == 8
    hist, excess, residual = CL.redistribute(np.bincount(img.ravel(), minlength=256), 8)
    assert (excess, residual) == (1016, 248)
    want = np.full(256, 4)
    want[248:] = 3
    want[77] = 12
    assert np.array_equal(hist, want) and hist.sum() == 1024
    assert CL.luts(img, (1, 1), 2.0)[0, 0, 77] == 80
    out = CL.clahe(img, (1, 1), 2.0)
    assert np.array_equal(out, np.full((32, 32), 80, np.uint8))
    out4 = CL.clahe(img, (4, 4), 2.0)    # (every tile has the same table: the interpolation of equal values is that value)
    assert len(np.unique(out4)) == 1


def test_residual_with_a_step_above_one():
    """residual 100: step = 2, the bins 0, 2, ..., 198 gain one; residual 3: step 85, the bins 0, 85, 170"""
    h = np.zeros(256, np.int64)
    h[5] = 10 + 256 + 100
    out, excess, residual = CL.redistribute(h, 10)
    assert (excess, residual) == (356, 100)
    want = np.ones(256, np.int64)
    want[0:200:2] += 1
    want[5] += 10
    assert np.array_equal(out, want)
    h[5] = 10 + 3
    out, excess, residual = CL.redistribute(h, 10)
    want = np.zeros(256, np.int64)
    want[[0, 85, 170]] = 1
    want[5] += 10
    assert residual == 3 and np.array_equal(out, want)
    h[5] = 10 + 512
    out, excess, residual = CL.redistribute(h, 10)
    assert residual == 0 and np.array_equal(out, np.full(256, 2) + 10 * (np.arange(256) == 5))


def test_one_tile_is_independent_of_position():
    """tiles 1 x 1: x1 = x2 = y1 = y2 = 0 after the clamp, so the four table values are one value t <= 255 and the fp32 result differs from t by a few
    ulps of 255 at most: rint gives t wherever the pixel is"""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (37, 53), dtype=np.uint8)
    L = CL.luts(img, (1, 1), 3.0)
    assert np.array_equal(CL.apply(img, L, (1, 1)), L[0, 0][img])


def test_weights_at_the_first_column_and_at_tile_centres():
    """tile_w = 8: x = 0 gives fx = -0.5, x1 = -1, xa = 0.5 -- and then both indices clamp to tile 0, so the pixel takes tile 0's table alone; x = 4 gives
    fx = 0, xa = 0: tile 0 alone; x = 12 gives fx = 1, xa = 0: tile 1 alone; x = 8 gives fx = 0.5: the mean of tiles 0 and 1"""
    x1, x2, xa, xa1 = CL.axis(64, 8, 8)
    assert (x1[0], x2[0], xa[0], xa1[0]) == (0, 0, 0.5, 0.5)
    assert (x1[4], x2[4], xa[4]) == (0, 1, 0.0) and (x1[12], x2[12], xa[12]) == (1, 2, 0.0)
    assert (x1[8], x2[8], xa[8]) == (0, 1, 0.5)
    assert (x1[63], x2[63]) == (7, 7)
    # an image whose left half is 10 and right half 200, tiles 2 x 1 of 8 x 4, no clipping: table 0 maps 10 -> 255 (every pixel is <= 10), 200 -> 255;
    # table 1 likewise 200 -> 255 and 10 -> 0 (no pixel of tile 1 is <= 10)
    img = np.zeros((4, 16), np.uint8)
    img[:, :8], img[:, 8:] = 10, 200
    L = CL.luts(img, (2, 1), 1e9)
    assert (L[0, 0, 10], L[0, 0, 200], L[0, 1, 10], L[0, 1, 200]) == (255, 255, 0, 255)
    v10 = np.full((4, 16), 10, np.uint8)
    out = CL.apply(v10, L, (2, 1))
    # x = 0 ... 4: table 0 alone = 255; x = 12 ... 15: table 1 alone = 0; between them 255 * (1 - xa): x = 8 -> xa = 0.5 -> 127.5 -> 128 (half to even)
    assert list(out[0, :5]) == [255] * 5 and list(out[0, 12:]) == [0] * 4
    assert out[0, 8] == 128 and out[0, 6] == int(np.rint(255 * 0.75)) and out[0, 10] == int(np.rint(255 * 0.25))


@pytest.mark.parametrize("W,tiles", [(65, 8), (63, 8), (97, 16), (95, 16)])
def test_the_mirror(W, tiles):
    """pads of tiles - 1 (65 / 8, 97 / 16) and of 1 (63 / 8, 95 / 16): the padded column x >= W is column 2 (W - 1) - x, the edge column is not repeated"""
    img = (np.arange(W, dtype=np.int64)[None, :] * 3 % 251).astype(np.uint8).repeat(tiles, 0)
    P = CL.pad(img, (tiles, tiles))
    padw = (-W) % tiles
    assert P.shape == (tiles, W + padw)
    for k in range(padw):
        assert np.array_equal(P[:, W + k], img[:, W - 2 - k])
    assert np.array_equal(P[:, :W], img)


def test_the_mirror_for_a_pad_of_one():
    img = np.arange(63 * 31, dtype=np.int64).reshape(31, 63).astype(np.uint8)
    P = CL.pad(img, (8, 4))
    assert P.shape == (32, 64)
    assert np.array_equal(P[:31, 63], img[:, 61]) and np.array_equal(P[31, :63], img[29, :]) and P[31, 63] == img[29, 61]
    assert CL.pad(img[:, :56], (8, 1)).shape == (31, 56)     # a dimension that divides is not padded


# ---- lvt_amd_equalisation_plan against plan ----------------------------------------------------------------------------------------------------
def test_the_librarys_plan_equals_the_definition(hip_lib):
    assert "lvt_amd_equalisation_plan" in hip_lib.ABI_SYMBOLS
    floor_seen = full_seen = False
    for (W, H), tiles in SIZES:
        for clip in CLIPS:
            got = hip_lib.equalisation_plan(hip_lib.Equalisation(tiles, clip), W, H)
            want = CL.plan(W, H, tiles, clip)
            assert got is not None, (W, H, tiles, clip)
            assert {k: got[k] for k in want if k != "lut_scale"} == {k: want[k] for k in want if k != "lut_scale"}, (W, H, tiles, clip, got, want)
            assert got["lut_scale"].tobytes() == want["lut_scale"].tobytes()
            floor_seen |= want["clip"] == 1
            full_seen |= want["clip"] == want["area"]
    assert floor_seen and full_seen
    assert CL.plan(1241, 376, (8, 8), 3.0) == {"Wp": 1248, "Hp": 376, "tile_w": 156, "tile_h": 47, "area": 7332, "clip": 85, "lut_scale": np.float32(255.0) / np.float32(7332)}


def test_the_plan_refuses_what_the_setter_refuses(hip_lib):
    E = hip_lib.Equalisation
    ok = hip_lib.equalisation_plan
    assert ok(E((8, 8), 3.0), 64, 64) is not None and ok(E((16, 1), 3.0), 16, 1) is not None
    for tiles in ((0, 8), (8, 0), (17, 8), (8, 17), (-1, 8)):
        assert ok(E(tiles, 3.0), 640, 480) is None, tiles
    assert ok(E((8, 8), 3.0), 7, 480) is None and ok(E((8, 8), 3.0), 640, 7) is None     # more tiles than pixels
    for clip in (float("nan"), float("inf"), float("-inf"), 0.0, -1.0):
        assert ok(E((8, 8), clip), 640, 480) is None, clip
    L = hip_lib.load_library()
    out = (hip_lib.C.c_int * 6)()
    assert L.lvt_amd_equalisation_plan(None, 640, 480, out, None) == -1
    e = E((8, 8), 3.0)
    assert L.lvt_amd_equalisation_plan(hip_lib.C.byref(e), 640, 480, out, None) == 0 and list(out) == [640, 480, 80, 60, 4800, 56]


# ---- what the property is for: the oracle on a dimmed world --------------------------------------------------------------------------------------
GAIN, OFFSET, TILES, CLIP = 0.12, 10.0, (8, 4), 3.0     # the dimming of the low-light tests (tests/test_gpu_equalised_frames.py uses the same)


def dimmed_world(n=6):
    world, prm, _ = make_case("kitti", 0, size=(610, 185))
    dimmed = [tuple(CL.dim(np.ascontiguousarray(g), GAIN, OFFSET) for g in world.render_stereo(i)) for i in range(n)]
    return prm, dimmed, [tuple(CL.clahe(g, TILES, CLIP) for g in pair) for pair in dimmed]


def test_the_oracle_is_lost_on_dimmed_frames_and_tracks_them_equalised(oracle_lib):
    O = oracle_lib
    prm, dimmed, equalised = dimmed_world()
    states = {}
    for name, frames in (("dimmed", dimmed), ("equalised", equalised)):
        orc, st, nm = O.Oracle(prm, 1), [], []
        for pair in frames:
            orc.track(*pair)
            st.append(orc.status)
            nm.append(orc.counts()["n_matches"])
        print(name, "states", st, "matches", nm)
        states[name] = st
    assert 3 in states["dimmed"][:3], states["dimmed"]               # LOST by frame 2
    assert states["equalised"] == [2] * 6, states["equalised"]       # TRACKING on every frame
