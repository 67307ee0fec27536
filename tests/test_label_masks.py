"""Label masks, the CPU tier: the numpy restatement of the definition (label_mask_util.label_plane) on hand-checked answers, the facts about the unchanged oracle
under the sliding-label sequence that the GPU tier (test_gpu_label_masks.py) rests on, and the record's host-side checks that need no device.

The worlds are those of test_feature_masks.py: the KITTI-shaped world 71 at 621 x 187 (stereo, the left eye labelled) and the TUM-shaped world 0 at 322 x 242
(RGB-D), 8 frames each; label sizes the image's own, a quarter and 100 x 37; dilate 0 / 3 / 15: 18 combinations."""
import ctypes as C

import numpy as np
import pytest

import label_mask_util as LU
import mask_util as MU
from test_feature_masks import KITTI, TUM, world_of


def plane(lab, drop, dilate, W, H, static=None):
    """the restatement, held to the literal reading of the definition on the way"""
    lab = np.asarray(lab, np.uint8)
    m = LU.label_plane(lab, drop, dilate, W, H, static)
    assert np.array_equal(m, LU.label_plane_slow(lab, drop, dilate, W, H, static))
    return m


# ---- hand-checked answers ------------------------------------------------------------------------------------------------------------------------
def test_a_one_by_one_label_image():
    assert np.all(plane([[5]], [5], 0, 7, 3) == 0) and np.all(plane([[5]], [4], 15, 7, 3) == 255)


def test_seven_label_columns_over_ten_pixels():
    """lx(x) = (7 x) // 10 = 0 0 1 2 2 3 4 4 5 6: label columns 0, 2 and 4 own two pixels each"""
    lab = np.arange(7, dtype=np.uint8)[None, :]
    assert plane(lab, [2], 0, 10, 1).tolist() == [[255, 255, 255, 0, 0, 255, 255, 255, 255, 255]]
    assert plane(lab, [1, 6], 0, 10, 1).tolist() == [[255, 255, 0, 255, 255, 255, 255, 255, 255, 0]]
    assert plane(lab, [3], 1, 10, 1).tolist() == [[255, 255, 255, 255, 0, 0, 0, 255, 255, 255]]
    # rows: ly(y) = (3 y) // 4 = 0 0 1 2
    assert plane(np.array([[0], [1], [2]], np.uint8), [0], 0, 1, 4)[:, 0].tolist() == [0, 0, 255, 255]


def test_a_label_image_wider_than_the_image():
    """label_width 10 over W = 4: lx = 0 2 5 7 -- the columns between are never read"""
    lab = np.array([[0, 9, 1, 9, 9, 2, 9, 3, 9, 9]], np.uint8)
    assert plane(lab, [9], 0, 4, 1).tolist() == [[255] * 4]
    assert plane(lab, [1, 3], 0, 4, 1).tolist() == [[255, 0, 255, 0]]
    assert plane(np.array([[0], [7], [7], [1], [7]], np.uint8), [7], 0, 1, 2)[:, 0].tolist() == [255, 0]   # ly = 0, 2


@pytest.mark.parametrize("dilate", [0, 1, 15])
def test_a_forbidden_pixel_in_each_corner_is_clipped_not_wrapped(dilate):
    W, H = 40, 36
    for cx, cy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
        lab = np.zeros((H, W), np.uint8)
        lab[cy, cx] = 1
        m = plane(lab, [1], dilate, W, H)
        y, x = np.mgrid[0:H, 0:W]
        want = np.where((abs(x - cx) <= dilate) & (abs(y - cy) <= dilate), 0, 255)
        assert np.array_equal(m, want), (cx, cy, dilate)
        assert (m == 0).sum() == (dilate + 1) ** 2, "the window is cut at the image's edge: a quarter of it remains, nothing appears on the far side"


def test_and_with_a_static_mask():
    lab = np.zeros((4, 6), np.uint8)
    lab[1, 2] = 3
    static = np.full((4, 6), 9, np.uint8)
    static[:, 5] = 0
    m = plane(lab, [3], 0, 6, 4, static)
    want = np.full((4, 6), 255, np.uint8)
    want[1, 2] = 0
    want[:, 5] = 0
    assert np.array_equal(m, want)
    assert np.all(plane(lab, [3], 0, 6, 4, np.zeros((4, 6), np.uint8)) == 0)


def test_an_empty_and_a_full_drop_set():
    rng = np.random.default_rng(1)
    lab = rng.integers(0, 256, (9, 13)).astype(np.uint8)
    assert np.all(plane(lab, [], 15, 20, 11) == 255) and np.all(plane(lab, range(256), 0, 20, 11) == 0)
    assert np.all(plane(lab, [True] * 256, 0, 20, 11) == 0) and np.all(plane(lab, [False] * 256, 3, 20, 11) == 255)


def test_the_restatement_on_random_cases():
    rng = np.random.default_rng(2)
    for W, H, LW, LH, d in ((33, 17, 9, 5, 2), (20, 31, 40, 62, 4), (17, 9, 17, 9, 15), (5, 3, 100, 37, 1)):
        lab = rng.integers(0, 6, (LH, LW)).astype(np.uint8)
        static = np.where(rng.random((H, W)) < 0.8, 200, 0).astype(np.uint8)
        plane(lab, [1, 4], d, W, H, static)


# ---- the sliding sequence under the unchanged oracle ---------------------------------------------------------------------------------------------
def corners_kept(w, i, mask):
    """frame i's left / only eye: (the detector's corners the mask keeps, all of them)"""
    c = w.corners[i][0]
    return MU.filter_corners(c, mask), c


def decided_differently(corners, W, H, a, b):
    f = MU.border_kept(corners, W, H)
    return int((MU.keep_rule(f[:, 0], f[:, 1], a) != MU.keep_rule(f[:, 0], f[:, 1], b)).sum())


@pytest.mark.parametrize("dilate", LU.DILATES)
@pytest.mark.parametrize("size", ["full", "quarter", "100x37"])
@pytest.mark.parametrize("case", [KITTI, TUM], ids=["kitti", "tum"])
def test_the_sliding_labels_under_the_oracle(oracle_lib, case, size, dilate):
    """every frame drops at least 10 % of its features (counted behind the border filter) and the oracle is TRACKING on all 8 frames; at quarter resolution
    and dilate 0 and 3 -- where a label column is four pixels and the blocks move 24 and 16 pixels a frame: the combinations the GPU tier binds frames in flight
    on -- the PREVIOUS frame's labels would decide at least 5 features of every frame from 1 on differently, so a wrong binding cannot pass.  (At the image's own
    size the blocks move 6 and 4 pixels a frame and some frames have no feature in the strips that change: the figure is printed, not asserted.)"""
    w = world_of(case)
    labs, masks = LU.sliding_masks(w.W, w.H, LU.label_sizes(w.W, w.H)[size], dilate)
    orc, shares, diffs, matches = oracle_lib.Oracle(w.prm, w.sensor), [], [], []
    for i in range(LU.N_FRAMES):
        kept, allc = corners_kept(w, i, masks[i])
        shares.append(MU.dropped_share(allc, masks[i], f"frame {i}", 0.10))
        if i:
            diffs.append(decided_differently(allc, w.W, w.H, masks[i], masks[i - 1]))
        if w.sensor == 1:
            L, R = w.frames[i]
            orc.track_with_external_corners(L, R, kept[:, :2].astype(np.float64), w.corners[i][1][:, :2].astype(np.float64))
        else:
            g, d = w.frames[i]
            orc.track_rgbd(g, MU.masked_depth(d, masks[i]))
        assert orc.status == 2, f"the oracle is not TRACKING at frame {i}"
        matches.append(orc.counts()["n_matches"])
    print(case[0], size, dilate, "dropped", [round(s, 2) for s in shares], "decided differently by the previous labels", diffs, "matches", matches[1:])
    if size == "quarter" and dilate in (0, 3):
        assert min(diffs) >= 5, diffs


# ---- the record's host-side checks: no device is touched ---------------------------------------------------------------------------------------------
def test_the_record_and_its_refusals_without_a_device(hip_lib):
    L = hip_lib.load_library()
    assert C.sizeof(hip_lib.LabelMask) == 268
    rec = hip_lib.LabelMask(100, 37, [11, 13], 3)
    assert (rec.label_width, rec.label_height, rec.dilate, rec.dropped()) == (100, 37, 3, [11, 13])
    assert hip_lib.LabelMask(4, 4, [0] * 255 + [1]).dropped() == [255]
    for name in ("lvt_amd_set_label_mask", "lvt_amd_batch_set_label_mask", "lvt_amd_get_label_mask", "lvt_amd_frame_labels", "lvt_amd_frame_labels_device",
                 "lvt_amd_build_label_mask"):
        assert name in hip_lib.ABI_SYMBOLS and hasattr(L, name)
    # a bad handle: -1, no report, no device
    assert L.lvt_amd_set_label_mask(None, C.byref(rec)) == -1 and L.lvt_amd_batch_set_label_mask(None, 0, C.byref(rec)) == -1
    assert L.lvt_amd_get_label_mask(None, 0, None) == -1
    lab = np.zeros((37, 100), np.uint8)
    assert L.lvt_amd_frame_labels(None, 0, lab.ctypes.data_as(C.c_void_p), None) == -1
    assert L.lvt_amd_frame_labels_device(None, 0, None, 0, None, 0) == -1
    # the stage entry refuses a bad record with a sentence that names the field and its limits, before it touches a device
    out = np.zeros((8, 64), np.uint8)
    p, o = lab.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for field, value, said in (("label_width", 0, "label_width = 0 (1 ... 8192)"), ("label_width", 8193, "label_width = 8193 (1 ... 8192)"),
                               ("label_height", -2, "label_height = -2 (1 ... 8192)"), ("dilate", 16, "dilate = 16 (0 ... 15)"), ("dilate", -1, "dilate = -1 (0 ... 15)")):
        bad = hip_lib.LabelMask(100, 37, [1], 0)
        setattr(bad, field, value)
        assert L.lvt_amd_build_label_mask(C.byref(bad), p, 8200, 40, 8, None, 0, o, 64) == -1
        err = L.lvt_amd_last_error(None).decode()
        assert err == "lvt_amd_build_label_mask: a label mask with " + said + " (nothing was changed)", err
    for args in ((None, p, 100, 40, 8, None, 0, o, 64), (C.byref(rec), None, 100, 40, 8, None, 0, o, 64),
                 (C.byref(rec), p, 100, 0, 8, None, 0, o, 64), (C.byref(rec), p, 100, 40, 8, None, 0, o, 39),
                 (C.byref(rec), p, 100, 40, 8, None, 0, o, 42), (C.byref(rec), p, 100, 40, 8, p, 39, o, 64),
                 (C.byref(rec), p, 99, 40, 8, None, 0, o, 64)):
        assert L.lvt_amd_build_label_mask(*args) == -1
        err = L.lvt_amd_last_error(None).decode()
        assert err.startswith("lvt_amd_build_label_mask: ") and err.endswith("(nothing was changed)"), err

