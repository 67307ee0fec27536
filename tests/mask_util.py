"""Feature masks: the numpy restatement of the rule (include/lvt_amd_ext.h, FEATURE MASKS), the three masks the tests use, and the two routes by which the
unchanged oracle tracks a masked frame.  No expected value comes from the library under test.

THE RULE, for every feature the gather step kept, in its output order:
    ix = (int)(bx + 0.5f);  iy = (int)(by + 0.5f)        -- fp32 add, then truncation (cv::KeyPointsFilter::runByPixelsMask)
    keep = 0 <= ix < W && 0 <= iy < H && mask[iy][ix] != 0
Truncation sends exactly the fp32 sums in (-1, W) to 0 ... W - 1, so the range test is made on the sum: no conversion leaves the range of an integer.

THE TWO EQUIVALENCES.  Stereo: a masked frame equals Oracle.track_with_external_corners(L, R, cl, cr) with cl, cr = O.detect_grid of each eye filtered by
the rule -- detect_grid includes the retry, which is decided on the unmasked count, and the border filter commutes with the mask.  The oracle gives external
corners the response 0, so feature `resp` is held to detect_grid's filtered third column instead.  RGB-D: detected corners are integers, so a masked frame
equals Oracle.track_rgbd(gray, where(mask != 0, depth, 0)): a zero depth fails the near-plane test."""
import numpy as np

HALF = np.float32(0.5)


def keep_rule(bx, by, mask):
    """bool array: the rule on fp32 coordinates (bx, by) against a (H, W) mask"""
    mask = np.asarray(mask)
    H, W = mask.shape
    fx = np.asarray(bx, dtype=np.float32).ravel() + HALF
    fy = np.asarray(by, dtype=np.float32).ravel() + HALF
    assert fx.dtype == np.float32 and fy.dtype == np.float32
    with np.errstate(invalid="ignore"):
        inside = (fx > np.float32(-1)) & (fx < np.float32(W)) & (fy > np.float32(-1)) & (fy < np.float32(H))
    keep = np.zeros(fx.shape, dtype=bool)
    ix, iy = np.trunc(fx[inside]).astype(np.int64), np.trunc(fy[inside]).astype(np.int64)
    keep[inside] = mask[iy, ix] != 0
    return keep


def filter_corners(xyr, mask):
    """the rows of an (n, >= 2) corner array the rule keeps, in order"""
    xyr = np.asarray(xyr)
    return xyr[keep_rule(xyr[:, 0], xyr[:, 1], mask)] if len(xyr) else xyr


# ---- the three masks -----------------------------------------------------------------------------------------------------------------------
def bonnet(W, H):
    """rows below 0.7 H zero: the ego vehicle's bonnet at the bottom of the frame"""
    m = np.full((H, W), 255, np.uint8)
    m[int(0.7 * H):] = 0
    return m


def checkerboard(W, H, cell=32, value=7):
    """32-px squares, `value` in the kept ones -- those whose column and row numbers have an odd sum -- (a mask byte is tested against zero, not against 255)"""
    y, x = np.mgrid[0:H, 0:W]
    return np.where(((x // cell) + (y // cell)) % 2 == 1, value, 0).astype(np.uint8)


def ellipse(W, H):
    """a centred ellipse with half axes 0.45 W and 0.55 H kept: the black surround of a wide-angle lens"""
    y, x = np.mgrid[0:H, 0:W]
    u, v = (x - W / 2.0) / (0.45 * W), (y - H / 2.0) / (0.55 * H)
    return np.where(u * u + v * v <= 1.0, 255, 0).astype(np.uint8)


MASKS = {"bonnet": bonnet, "checkerboard": checkerboard, "ellipse": ellipse}
MIN_SHARE = {"bonnet": 0.10, "checkerboard": 0.10, "ellipse": 0.0}   # of a frame's features a mask must drop in every frame and eye it is compared on


def border_kept(xyr, W, H, B=28):
    """the corners BRIEF's border filter keeps (cvRound, 28 px): the features a frame has before the mask acts"""
    xyr = np.asarray(xyr)
    ix, iy = np.rint(xyr[:, 0]), np.rint(xyr[:, 1])
    return xyr[(ix >= B) & (ix < W - B) & (iy >= B) & (iy < H - B)]


def dropped_share(corners, mask, what, at_least=0.0):
    """the share of the features among `corners` (those behind the border filter) the mask drops; asserts that it drops at least one, and at least
    `at_least` of them"""
    corners = border_kept(corners, mask.shape[1], mask.shape[0])
    n = len(corners)
    k = int(keep_rule(corners[:, 0], corners[:, 1], mask).sum()) if n else 0
    assert n > 0 and k < n, f"{what}: the mask drops none of the {n} corners -- the case compares nothing"
    share = (n - k) / n
    assert share >= at_least, f"{what}: the mask drops {share:.1%} of the corners, the case needs {at_least:.0%}"
    return share


# ---- the oracle's routes ---------------------------------------------------------------------------------------------------------------------
def masked_corners(img, prm, mask):
    """(corners the oracle's detector finds in img and the mask keeps [n x 3: x, y, response], all corners it finds) -- mask None keeps all"""
    from oracle import pyoracle as O
    xyr, _ = O.detect_grid(img, prm)
    return (xyr if mask is None else filter_corners(xyr, mask)), xyr


def oracle_track_masked(orc, prm, L, R, mask_l, mask_r, what="", at_least=0.0):
    """one masked stereo frame through the oracle's external-corner route.  Returns (R, t, (resp_l, resp_r)): the responses the kept corners of each eye have
    BEHIND the border filter (what the tracker reports for them).  Asserts that every mask given drops a corner."""
    kept = []
    for eye, (img, m) in enumerate(((L, mask_l), (R, mask_r))):
        k, allc = masked_corners(img, prm, m)
        if m is not None:
            dropped_share(allc, m, f"{what} eye {eye}", at_least)
        kept.append(k)
    Ro, to = orc.track_with_external_corners(L, R, kept[0][:, :2].astype(np.float64), kept[1][:, :2].astype(np.float64))
    resp = []
    for eye in (0, 1):
        xy = orc.features(eye)[0]
        resp.append(responses_of(kept[eye], xy))
    return Ro, to, tuple(resp)


def responses_of(xyr, xy):
    """the responses of the features `xy` (a subsequence of the corner list xyr, in order): matched by walking both lists once"""
    out, j = np.zeros(len(xy), np.float32), 0
    for i in range(len(xy)):
        while j < len(xyr) and not (xyr[j, 0] == xy[i, 0] and xyr[j, 1] == xy[i, 1]):
            j += 1
        assert j < len(xyr), "a feature that is no corner of the list it was made from"
        out[i] = xyr[j, 2]
        j += 1
    return out


def diff_frame_but_resp(hip, orc, resp):
    """parity_util.diff_frame without the features' responses (the oracle's external corners have none), which are held to `resp` instead"""
    from parity_util import diff_frame
    msgs = [m for m in diff_frame(hip, orc) if ".resp" not in m]
    for eye in (0, 1):
        rh = hip.features(eye)[1]
        if rh.shape != resp[eye].shape or not np.array_equal(rh, resp[eye]):
            msgs.append(f"features[{eye}].resp differs from the detector's responses of the kept corners")
    return msgs


def masked_depth(depth, mask):
    return np.where(np.asarray(mask) != 0, depth, np.zeros_like(depth)).astype(depth.dtype)
