"""The definition of the equalisation (include/lvt_amd_ext.h, DIM frames) restated in numpy: integer arithmetic where the text says integer, one fp32
operation per written operation where it says fp32 (np.float32 scalars and arrays: numpy rounds every operation to fp32, np.rint rounds half to even).
Nothing here calls the library; tests/test_clahe.py holds this file to answers worked out by hand."""
import numpy as np

F = np.float32


def plan(W, H, tiles, clip_limit):
    """steps 1 and 2: {Wp, Hp, tile_w, tile_h, area, clip, lut_scale}"""
    tx, ty = tiles
    Wp, Hp = W + (-W) % tx, H + (-H) % ty
    tile_w, tile_h = Wp // tx, Hp // ty
    area = tile_w * tile_h
    with np.errstate(over="ignore"):
        c = F(F(clip_limit) * F(area)) / F(256.0)
    clip = area if c >= F(area) else max(int(c), 1)
    return {"Wp": Wp, "Hp": Hp, "tile_w": tile_w, "tile_h": tile_h, "area": area, "clip": clip, "lut_scale": F(255.0) / F(area)}


def pad(img, tiles):
    """the Wp x Hp image: x >= W reads 2 (W - 1) - x, likewise y"""
    H, W = img.shape
    p = plan(W, H, tiles, 1.0)
    xs, ys = np.arange(p["Wp"]), np.arange(p["Hp"])
    xs = np.where(xs >= W, 2 * (W - 1) - xs, xs)
    ys = np.where(ys >= H, 2 * (H - 1) - ys, ys)
    return img[np.ix_(ys, xs)]


def redistribute(hist, clip):
    """step 3 on one 256-bin histogram (int64 in, int64 out)"""
    hist = np.asarray(hist, np.int64)
    excess = int(np.maximum(hist - clip, 0).sum())
    out = np.minimum(hist, clip)
    batch = excess // 256
    residual = excess - 256 * batch
    out = out + batch
    if residual > 0:
        step = max(256 // residual, 1)
        i, left = 0, residual
        while i < 256 and left > 0:
            out[i] += 1
            i += step
            left -= 1
    return out, excess, residual


def luts(img, tiles, clip_limit, stats=None):
    """steps 3 and 4: (tiles_y, tiles_x, 256) uint8.  stats (a list): one (excess, residual) per tile is appended"""
    H, W = img.shape
    p = plan(W, H, tiles, clip_limit)
    P = pad(img, tiles)
    tx, ty = tiles
    out = np.zeros((ty, tx, 256), np.uint8)
    for j in range(ty):
        for i in range(tx):
            t = P[j * p["tile_h"]:(j + 1) * p["tile_h"], i * p["tile_w"]:(i + 1) * p["tile_w"]]
            hist, excess, residual = redistribute(np.bincount(t.ravel(), minlength=256), p["clip"])
            if stats is not None:
                stats.append((excess, residual))
            cum = np.cumsum(hist)
            v = np.rint(cum.astype(np.float32) * p["lut_scale"])    # (int64 -> float32 rounds to nearest even)
            out[j, i] = np.clip(v, 0, 255).astype(np.uint8)
    return out


def axis(n, tile, tiles):
    """step 5 along one axis for positions 0 ... n - 1: (t1, t2, a, a1), the indices clamped AFTER a is taken"""
    f = np.arange(n).astype(np.float32) * (F(1.0) / F(tile)) - F(0.5)
    fl = np.floor(f)
    a = f - fl
    a1 = F(1.0) - a
    t1 = fl.astype(np.int64)
    return np.clip(t1, 0, tiles - 1), np.clip(t1 + 1, 0, tiles - 1), a.astype(np.float32), a1.astype(np.float32)


def apply(img, L, tiles, clip_limit=1.0):
    """step 5: the equalised image from the tables L"""
    H, W = img.shape
    p = plan(W, H, tiles, clip_limit)
    x1, x2, xa, xa1 = axis(W, p["tile_w"], tiles[0])
    y1, y2, ya, ya1 = axis(H, p["tile_h"], tiles[1])
    v = img.astype(np.int64)
    Y1, Y2 = y1[:, None], y2[:, None]
    X1, X2 = x1[None, :], x2[None, :]
    XA, XA1, YA, YA1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    g = lambda yy, xx: L[yy, xx, v].astype(np.float32)    # noqa: E731
    top = g(Y1, X1) * XA1 + g(Y1, X2) * XA
    bot = g(Y2, X1) * XA1 + g(Y2, X2) * XA
    r = top * YA1 + bot * YA
    assert r.dtype == np.float32
    return np.clip(np.rint(r), 0, 255).astype(np.uint8)


def clahe(img, tiles=(8, 8), clip_limit=3.0):
    img = np.ascontiguousarray(img, np.uint8)
    return apply(img, luts(img, tiles, clip_limit), tiles, clip_limit)


def dim(img, gain=0.12, offset=10.0):
    """the dimming of the low-light tests: clip(rint(gain * g + offset))"""
    return np.clip(np.rint(gain * img.astype(np.float64) + offset), 0, 255).astype(np.uint8)
