"""Label masks: the numpy restatement of the definition (include/lvt_amd_ext.h, LABEL MASKS) and the sliding-label sequence the tests use.  No expected value
comes from the library under test.

THE DEFINITION, pure integer arithmetic.  A label image `lab` of label_width x label_height, a drop set, a dilation in pixels of the W x H detector grid:
    lx(x) = (x * label_width) // W        ly(y) = (y * label_height) // H
    f0(x, y) = drop[lab[ly(y)][lx(x)]] != 0
    f(x, y)  = OR of f0(x', y') over |x' - x| <= dilate, |y' - y| <= dilate, 0 <= x' < W, 0 <= y' < H       -- a square window, clipped, never wrapped
    m(x, y)  = 255 if not f(x, y) and (no static mask or static[y][x] != 0) else 0
m is an ordinary feature mask: mask_util.keep_rule filters key points with it."""
import numpy as np

DROPPED = (11, 13)      # the labels the sliding sequence forbids
EVERYWHERE = 7
N_FRAMES = 8
DILATES = (0, 3, 15)


def drop_flags(drop):
    """256 bools from an iterable of label values (or 256 flags)"""
    drop = list(drop)
    if len(drop) == 256:
        return np.array([bool(v) for v in drop])
    flags = np.zeros(256, bool)
    flags[[int(l) for l in drop]] = True
    return flags


def forbidden0(lab, drop, W, H):
    """f0: (H, W) bool"""
    lab = np.asarray(lab)
    assert lab.dtype == np.uint8 and lab.ndim == 2
    LH, LW = lab.shape
    lx = (np.arange(W, dtype=np.int64) * LW) // W
    ly = (np.arange(H, dtype=np.int64) * LH) // H
    return drop_flags(drop)[lab[np.ix_(ly, lx)]]


def dilated(f0, dilate):
    """f: the OR over the clipped square window, one axis after the other (the square is separable)"""
    f = np.array(f0, dtype=bool)
    for axis in (1, 0):
        acc = f.copy()
        for k in range(1, int(dilate) + 1):
            a, b = [slice(None)] * 2, [slice(None)] * 2
            a[axis], b[axis] = slice(k, None), slice(None, -k)
            if f.shape[axis] > k:
                acc[tuple(b)] |= f[tuple(a)]      # pixel p sees p + k
                acc[tuple(a)] |= f[tuple(b)]      # pixel p sees p - k
        f = acc
    return f


def label_plane(lab, drop, dilate, W, H, static=None):
    """m: the (H, W) uint8 plane, 255 allowed / 0 forbidden"""
    ok = ~dilated(forbidden0(lab, drop, W, H), dilate)
    if static is not None:
        static = np.asarray(static)
        assert static.shape == (H, W)
        ok &= static != 0
    return np.where(ok, 255, 0).astype(np.uint8)


def label_plane_slow(lab, drop, dilate, W, H, static=None):
    """the definition read literally, window by window: what label_plane is held to on small images"""
    f0 = forbidden0(lab, drop, W, H)
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            f = f0[max(0, y - dilate):min(H, y + dilate + 1), max(0, x - dilate):min(W, x + dilate + 1)].any()
            out[y, x] = 255 if (not f and (static is None or static[y, x] != 0)) else 0
    return out


# ---- the sliding-label sequence -----------------------------------------------------------------------------------------------------------------
def sliding_labels(LW, LH, i):
    """frame i's label image: label 7 everywhere; a block of label 13 over rows 0.3 ... 0.9 of the height, starting at column 0.10 LW + 6 i and 0.22 LW wide;
    a block of label 11 over rows 0.4 ... 0.8, starting at column 0.80 LW - 4 i and 0.06 LW wide (columns are cut at the image's edge)"""
    lab = np.full((LH, LW), EVERYWHERE, np.uint8)

    def block(r0, r1, c0, w, label):
        c0, c1 = max(0, min(LW, c0)), max(0, min(LW, c0 + max(1, w)))
        lab[int(r0 * LH):max(int(r0 * LH) + 1, int(r1 * LH)), c0:c1] = label
    block(0.3, 0.9, int(0.10 * LW) + 6 * i, int(0.22 * LW), 13)
    block(0.4, 0.8, int(0.80 * LW) - 4 * i, int(0.06 * LW), 11)
    return lab


def label_sizes(W, H):
    """the three label sizes of the sequence tests: the image's own, a quarter, and 100 x 37"""
    return {"full": (W, H), "quarter": ((W + 3) // 4, (H + 3) // 4), "100x37": (100, 37)}


def sliding_masks(W, H, size, dilate, static=None, n=N_FRAMES):
    """([label image of frame i], [its plane m]) for a label size (LW, LH)"""
    labs = [sliding_labels(size[0], size[1], i) for i in range(n)]
    return labs, [label_plane(l, DROPPED, dilate, W, H, static) for l in labs]
