"""SENSOR FORMATS in numpy: the definition of include/lvt_amd_ext.h restated on integers, and the inputs the sensor-format tests share.  Nothing here comes
from the library under test: planes are converted HERE and the unchanged oracle is fed the converted frames."""
import numpy as np

NONE, RGGB, BGGR, GRBG, GBRG, YUYV, UYVY, MONO16 = 0, 16, 17, 18, 19, 24, 25, 32
BAYER = (RGGB, BGGR, GRBG, GBRG)
FORMATS = BAYER + (YUYV, UYVY, MONO16)
NAMES = {RGGB: "RGGB8", BGGR: "BGGR8", GRBG: "GRBG8", GBRG: "GBRG8", YUYV: "YUYV", UYVY: "UYVY", MONO16: "MONO16"}
BPP = {RGGB: 1, BGGR: 1, GRBG: 1, GBRG: 1, YUYV: 2, UYVY: 2, MONO16: 2}
# the pattern names the colours of pixels (0,0), (1,0) / (0,1), (1,1): RED[fmt] = (x parity, y parity) of the red sample; blue sits on the other diagonal end
RED = {RGGB: (0, 0), BGGR: (1, 1), GRBG: (1, 0), GBRG: (0, 1)}
EVERY_VALUE_WINDOWS = [(0, 65535), (0, 1), (65534, 65535), (1000, 1300), (4096, 8191)]


def mirror_pad(a):
    """one pixel all round, mirrored WITHOUT repeating the edge: -1 -> 1, n -> n - 2 (numpy's 'reflect'); every side is at least 2"""
    assert a.ndim == 2 and min(a.shape) >= 2
    return np.pad(a, 1, mode="reflect")


def bayer_planes(m, fmt):
    """(R4, G4, B4) of a mosaic: 4 x each channel at every pixel, the missing ones as the unscaled mean of the nearest samples of that colour"""
    m = np.asarray(m)
    assert m.dtype == np.uint8 and m.ndim == 2
    H, W = m.shape
    p = mirror_pad(m).astype(np.int64)
    c = p[1:-1, 1:-1]
    hs = p[1:-1, :-2] + p[1:-1, 2:]                       # left + right
    vs = p[:-2, 1:-1] + p[2:, 1:-1]                       # above + below
    ds = p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:]  # the four diagonals
    rx, ry = RED[fmt]
    y, x = np.mgrid[0:H, 0:W]
    red_row, red_col = (y & 1) == ry, (x & 1) == rx
    at_red, at_blue = red_row & red_col, ~red_row & ~red_col
    R4 = np.where(at_red, 4 * c, np.where(at_blue, ds, np.where(red_row, 2 * hs, 2 * vs)))
    B4 = np.where(at_blue, 4 * c, np.where(at_red, ds, np.where(red_row, 2 * vs, 2 * hs)))
    G4 = np.where(at_red | at_blue, hs + vs, 4 * c)
    return R4, G4, B4


def bayer_to_gray(m, fmt):
    """gray = (4899 R4 + 9617 G4 + 1868 B4 + 32768) >> 16: one rounding.  With X4 = 4 X exactly (a mosaic of an image that is constant per channel) this
    is (4 s + 32768) >> 16 == (s + 8192) >> 14 for s = 4899 R + 9617 G + 1868 B: colour_util.gray_of_rgb(R, G, B), exactly"""
    R4, G4, B4 = bayer_planes(m, fmt)
    s = 4899 * R4 + 9617 * G4 + 1868 * B4 + 32768
    assert s.max() <= 16744448
    return np.ascontiguousarray((s >> 16).astype(np.uint8))


def mosaic(r, g, b, fmt):
    """the Bayer mosaic of a colour image: every pixel keeps the one channel its site samples"""
    r, g, b = (np.asarray(a, np.uint8) for a in (r, g, b))
    H, W = r.shape
    rx, ry = RED[fmt]
    y, x = np.mgrid[0:H, 0:W]
    red_row, red_col = (y & 1) == ry, (x & 1) == rx
    return np.ascontiguousarray(np.where(red_row & red_col, r, np.where(~red_row & ~red_col, b, g)).astype(np.uint8))


def yuv422_to_gray(rows, fmt):
    """(H, 2 W) bytes -> (H, W): every second byte, from 0 (YUYV) or 1 (UYVY); no range expansion"""
    rows = np.asarray(rows)
    assert rows.dtype == np.uint8 and rows.ndim == 2 and rows.shape[1] % 2 == 0
    return np.ascontiguousarray(rows[:, (0 if fmt == YUYV else 1)::2])


def yuv422_of_gray(g, fmt, seed=0):
    """a 4:2:2 plane whose luma is g; the chroma bytes are random"""
    g = np.asarray(g, np.uint8)
    out = np.random.default_rng(seed).integers(0, 256, size=(g.shape[0], 2 * g.shape[1]), dtype=np.uint8)
    out[:, (0 if fmt == YUYV else 1)::2] = g
    return out


def map16(v, lo, hi):
    """g = min(max(v, lo), hi); out = ((g - lo) 255 + ((hi - lo) >> 1)) // (hi - lo)"""
    assert 0 <= lo < hi <= 65535
    g = np.clip(np.asarray(v).astype(np.int64), lo, hi)
    return (((g - lo) * 255 + ((hi - lo) >> 1)) // (hi - lo)).astype(np.uint8)


def auto_window(v, lo_pm, hi_pm, min_span):
    """(lo, hi) from the histogram of v >> 4 (4096 bins) over all pixels of one image; Python integers, so the products cannot overflow"""
    v = np.asarray(v)
    assert v.dtype == np.uint16 and 0 <= lo_pm <= 499 and 0 <= hi_pm <= 499 and 1 <= min_span <= 65535
    cum = np.cumsum(np.bincount((v >> 4).reshape(-1), minlength=4096)).tolist()
    N = int(v.size)
    lo_bin = next(b for b in range(4096) if cum[b] * 1000 > lo_pm * N)
    hi_bin = next(b for b in range(4096) if cum[b] * 1000 >= (1000 - hi_pm) * N)
    lo, hi = 16 * lo_bin, 16 * hi_bin + 15
    if hi - lo < min_span:
        mid = (lo + hi) >> 1
        lo = max(0, mid - (min_span >> 1))
        hi = lo + min_span
        if hi > 65535:
            hi = 65535
            lo = hi - min_span
    return lo, hi


class Record:
    """a sensor-format record as plain Python (tests build the library's SensorFormat from its fields)"""

    def __init__(self, format, auto_window=0, lo=0, hi=65535, lo_permille=0, hi_permille=0, min_span=1):
        self.format, self.auto_window, self.lo, self.hi = format, auto_window, lo, hi
        self.lo_permille, self.hi_permille, self.min_span = lo_permille, hi_permille, min_span

    def fields(self):
        return dict(format=self.format, auto_window=self.auto_window, lo=self.lo, hi=self.hi, lo_permille=self.lo_permille, hi_permille=self.hi_permille,
                    min_span=self.min_span)


def convert(plane, rec):
    """(gray (H, W) uint8, window or None) of a sensor's plane: (H, W) u8 Bayer, (H, 2 W) u8 YUV 4:2:2, (H, W) u16 MONO16"""
    if rec.format in BAYER:
        return bayer_to_gray(plane, rec.format), None
    if rec.format in (YUYV, UYVY):
        return yuv422_to_gray(plane, rec.format), None
    assert rec.format == MONO16 and plane.dtype == np.uint16
    lo, hi = auto_window(plane, rec.lo_permille, rec.hi_permille, rec.min_span) if rec.auto_window else (rec.lo, rec.hi)
    return np.ascontiguousarray(map16(plane, lo, hi)), (lo, hi)


def thermal(gray, seed):
    """a 'thermal' rendering of a gray frame: 20000 + 3 g plus integer noise in [-2, 2], uint16 -- the scene spans under 800 of 65 536 counts"""
    rng = np.random.default_rng([20000, int(seed)])
    return np.ascontiguousarray((20000 + 3 * gray.astype(np.int64) + rng.integers(-2, 3, size=gray.shape)).astype(np.uint16))


THERMAL = Record(MONO16, auto_window=1, lo_permille=5, hi_permille=5, min_span=256)


def planted_histograms():
    """[(name, image u16 (H, W), (lo_pm, hi_pm, min_span), expected window worked out by hand)]"""
    out = []
    one = np.full((8, 25), 0x1234, np.uint16)                      # all 200 pixels in bin 0x123: [0x1230, 0x123F], span 15
    out.append(("one-bin-span-decides", one, (0, 0, 100), (0x1237 - 50, 0x1237 - 50 + 100)))
    out.append(("one-bin-span-small", one, (10, 10, 15), (0x1230, 0x123F)))
    out.append(("one-bin-bottom", np.full((8, 25), 3, np.uint16), (0, 0, 1000), (0, 1000)))             # mid = 7: lo clamps at 0
    out.append(("one-bin-top", np.full((8, 25), 65535, np.uint16), (0, 0, 1000), (64535, 65535)))      # [65520, 65535]: hi clamps at 65535
    # 1000 pixels, lo_permille = 100: exactly 100 pixels below (bin 2) do NOT move lo past them ... (cum * 1000 > 100 * 1000 fails at bin 2 only if cum <= 100)
    exact = np.full(1000, 16 * 50 + 1, np.uint16)
    exact[:100] = 16 * 2
    exact[-100:] = 16 * 90
    out.append(("exactly-the-share", exact.reshape(20, 50).copy(), (100, 100, 1), (16 * 50, 16 * 50 + 15)))
    more = exact.copy()
    more[100] = 16 * 2                                             # one pixel more below: 101 > 100, lo stays at bin 2
    more[-101] = 16 * 90                                           # ... and above: bins <= 50 hold 798 < 900, hi goes to bin 90
    out.append(("one-pixel-more", more.reshape(20, 50).copy(), (100, 100, 1), (16 * 2, 16 * 90 + 15)))
    out.append(("permille-zero", exact.reshape(20, 50).copy(), (0, 0, 1), (16 * 2, 16 * 90 + 15)))
    return out


def every_value_image():
    """256 x 256 uint16: every v in 0 ... 65 535 once"""
    return np.arange(65536, dtype=np.uint16).reshape(256, 256).copy()
