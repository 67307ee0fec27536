"""Planted inputs for the rectifier: every place where the remap's arithmetic branches ("RECTIFICATION", include/lvt_amd_ext.h), at the smallest shapes that
carry it.  CASES maps "group/name" to (source, map1, map2); the maps are built by formula from small integers over powers of two, so every planted value is
exact in fp32 (what is planted is what the kernel reads).  CALIBRATIONS maps a name to (K, D, R, P, w, h) for the map builder.  Nothing here is random
except where a group says so, and then from a fixed seed."""
import numpy as np

F32 = np.float32
BENIGN = 1.25   # an entry well inside every source that is at least 3 wide or high: filler of a case's last row


def _maps(pairs, dw):
    """a list of (mx, my) entries as two (dh, dw) maps, the last row filled up with BENIGN"""
    pairs = list(pairs)
    dh = (len(pairs) + dw - 1) // dw
    pairs += [(BENIGN, BENIGN)] * (dh * dw - len(pairs))
    a = np.array(pairs, np.float64)
    m1, m2 = a[:, 0].astype(F32).reshape(dh, dw), a[:, 1].astype(F32).reshape(dh, dw)
    exact = (np.isnan(a[:, 0]) | (m1.reshape(-1).astype(np.float64) == a[:, 0])) & (np.isnan(a[:, 1]) | (m2.reshape(-1).astype(np.float64) == a[:, 1]))
    assert exact.all(), "a planted value is not exact in fp32"
    return m1, m2


def _noise(sw, sh, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (sh, sw), dtype=np.uint8)


def distinct_border(sw, sh):
    """a source whose border pixels are all different (and none of them 0), interior 7"""
    s = np.full((sh, sw), 7, np.uint8)
    border = [(0, x) for x in range(sw)] + [(sh - 1, x) for x in range(sw)] + [(y, 0) for y in range(1, sh - 1)] + [(y, sw - 1) for y in range(1, sh - 1)]
    assert len(border) < 120
    for k, (y, x) in enumerate(border):
        s[y, x] = 255 - 2 * k
    return s


CASES = {}

# ---- ties: m * 32 = k + 0.5 exactly, k even and odd, positive and negative; in x, in y, in both -------------------------------------------------------------
_TIE_K = [-41, -40, -34, -33, -32, -31, -3, -2, -1, 0, 1, 2, 31, 32, 33, 64, 65, 126, 127, 200, 201, 254, 255]
_tie = lambda k: (2 * k + 1) / 64.0   # noqa: E731
CASES["ties/x"] = (_noise(12, 10, 1), *_maps([(_tie(k), 3.25) for k in _TIE_K], 5))
CASES["ties/y"] = (_noise(10, 12, 2), *_maps([(3.25, _tie(k)) for k in _TIE_K], 5))
CASES["ties/both"] = (_noise(12, 12, 3), *_maps([(_tie(a), _tie(b)) for a in _TIE_K[::2] for b in _TIE_K[1::2]], 7))

# ---- negative: fixed-point values -1 ... -64, that is entries in (-2, 0) with every fraction 0 ... 31: the shift must floor, the mask stay non-negative --------
_NEG = [-k / 32.0 for k in range(1, 65)]
CASES["negative/x"] = (_noise(5, 4, 4, 128), *_maps([(m, y) for m in _NEG for y in (0.5, 2.0)], 9))
CASES["negative/y"] = (_noise(5, 4, 5, 128), *_maps([(x, m) for m in _NEG for x in (0.5, 2.0)], 9))
CASES["negative/both"] = (_noise(5, 4, 6, 128), *_maps([(a, b) for a in _NEG[::3] for b in _NEG[1::5]], 9))

# ---- edges: the eight partial places and the four places just outside, at four fractions each, on a 6 x 5 source with a border of different pixels -------------
_SW, _SH = 6, 5
_FR = [0.0, 1 / 32.0, 0.5, 31 / 32.0]
_cols = {"left": -1, "mid": 2, "right": _SW - 1, "out_left": -2, "out_right": _SW}
_rows = {"top": -1, "mid": 2, "bottom": _SH - 1, "out_top": -2, "out_bottom": _SH}
_edge = []
for _r in ("top", "mid", "bottom", "out_top", "out_bottom"):
    for _c in ("left", "mid", "right", "out_left", "out_right"):
        if (_r, _c) != ("mid", "mid"):
            _edge += [(_cols[_c] + fa, _rows[_r] + fb) for fa in _FR for fb in _FR]
CASES["edges/6x5"] = (distinct_border(_SW, _SH), *_maps(_edge, 11))

# ---- integer_255: all-integer entries (weights 32767, 0, 0, 1) on 255, 254 and 1, the source's last row and column (partial places) included -----------------
_I = np.array([[255, 254, 1, 255, 255], [1, 255, 254, 1, 255], [254, 1, 255, 255, 1], [255, 255, 1, 254, 255]], np.uint8)
CASES["integer_255/identity"] = (_I, *_maps([(float(x), float(y)) for y in range(4) for x in range(5)], 5))
CASES["integer_255/all_255"] = (np.full((3, 3), 255, np.uint8), *_maps([(float(x), float(y)) for y in range(-1, 4) for x in range(-1, 4)], 5))

# ---- fractions: all 32 x 32 weight pairs on the two 2 x 2 blocks that tell every weight apart ------------------------------------------------------------------
_fx = (np.arange(32, dtype=np.float64) / 32.0)
_F1, _F2 = np.tile(_fx[None, :], (32, 1)).astype(F32), np.tile(_fx[:, None], (1, 32)).astype(F32)
CASES["fractions/diagonal"] = (np.array([[255, 0], [0, 255]], np.uint8), _F1, _F2)
CASES["fractions/antidiagonal"] = (np.array([[0, 255], [255, 0]], np.uint8), _F1, _F2)
# (the same pairs one pixel into a 4 x 4 source: four different values, none of them at the source's origin)
CASES["fractions/inner"] = (np.array([[9, 9, 9, 9], [9, 255, 1, 9], [9, 2, 254, 9], [9, 9, 9, 9]], np.uint8), _F1 + F32(1), _F2 + F32(1))

# ---- clamp: the +-32768 clamp of the coarse coordinate -------------------------------------------------------------------------------------------------------
_CL = [32767.96875, 32768.0, 40000.0, 2.0 ** 20]     # (32767.97 is 32767 + 31/32 in fp32)
_CL = _CL + [-v for v in _CL]
CASES["clamp/small"] = (_noise(5, 4, 7, 100), *_maps([(v, 0.0) for v in _CL] + [(0.0, v) for v in _CL] + [(a, b) for a in _CL[::3] for b in _CL[1::3]], 7))
# (a source of 5 x 4 is outside with and without the clamp.  The clamp is cv::remap's saturation to short, and it shows only on a source wider or higher than
# 32768: there an entry of 32768.5 samples pixels 32767 and 32768, not 32768 and 32769)
_wide = (np.arange(32770) % 251 + 1).astype(np.uint8)
_CW = [32766.5, 32767.0, 32767.5, 32768.0, 32768.5, 32769.0, 32769.5, 32770.0, 40000.0]
CASES["clamp/wide_source"] = (_wide[None, :].copy(), *_maps([(v, 0.0) for v in _CW], 4))
CASES["clamp/high_source"] = (_wide[:, None].copy(), *_maps([(0.0, v) for v in _CW], 4))

# ---- extreme: entries the rule sends to INT_MIN, and their finite neighbours.  Pixel (0, 0) is 255, every other pixel below 100: a wrapped or zeroed
# conversion samples (0, 0) and shows; the answer is 0 on every planted pixel ------------------------------------------------------------------------------
_two26 = 2.0 ** 26
EXTREME = [float("nan"), float("inf"), -float("inf"), _two26, -_two26, 2.0 ** 27, -2.0 ** 27, 2.0 ** 31, -2.0 ** 31, 3e38, -3e38,
           float(np.nextafter(F32(_two26), F32(0))), float(np.nextafter(F32(_two26), F32(np.inf))),
           float(np.nextafter(F32(-_two26), F32(0))), float(np.nextafter(F32(-_two26), F32(-np.inf)))]
EXTREME = [float(F32(v)) for v in EXTREME]    # (3e38 as fp32 holds it)
_ex_src = _noise(6, 5, 8, 1, 100)
_ex_src[0, 0] = 255
EXTREME_PLANTED = 2 * len(EXTREME) + 9        # the first entries of the case, row after row: x with a benign y, y with a benign x, then pairs
CASES["extreme/6x5"] = (_ex_src, *_maps([(v, 0.0) for v in EXTREME] + [(0.0, v) for v in EXTREME] + [(a, b) for a in EXTREME[:3] for b in EXTREME[:3]], 7))

# ---- thin sources: no pixel can take the fast path (max(sw - 1, 0) == 0 or max(sh - 1, 0) == 0), under a 9 x 5 map sweeping -1.5 ... sw + 0.5 -----------------
for _sw, _sh in ((1, 1), (1, 7), (7, 1), (2, 2)):
    _mx = (-1.5 + np.arange(9) * (_sw + 2) / 8.0)
    _my = (-1.5 + np.arange(5) * (_sh + 2) / 4.0)
    CASES[f"thin_sources/{_sw}x{_sh}"] = (_noise(_sw, _sh, 10 + _sw + 3 * _sh, 200), np.tile(_mx[None, :], (5, 1)).astype(F32), np.tile(_my[:, None], (1, 9)).astype(F32))

# ---- narrow outputs: a row of one word that is part image, part padding; random maps (multiples of 1/64: ties included), about a third outside a 40 x 30 source --
for _dw in (1, 2, 3, 4, 5, 63, 64, 65):
    for _dh in (1, 2, 33):
        _rng = np.random.default_rng(1000 * _dw + _dh)
        _m1 = (_rng.integers(-6 * 64, 45 * 64, (_dh, _dw)) / 64.0).astype(F32)
        _m2 = (_rng.integers(-5 * 64, 34 * 64, (_dh, _dw)) / 64.0).astype(F32)
        CASES[f"narrow_outputs/{_dw}x{_dh}"] = (_noise(40, 30, 20), _m1, _m2)

# ---- zoom: the map's size is not the source's (entries rounded to 1/64 px) ------------------------------------------------------------------------------------
def _zoom(sw, sh, dw, dh):
    mx = np.rint(((np.arange(dw) + 0.5) * sw / dw - 0.5) * 64) / 64.0
    my = np.rint(((np.arange(dh) + 0.5) * sh / dh - 0.5) * 64) / 64.0
    return _noise(sw, sh, sw + dw), np.tile(mx[None, :], (dh, 1)).astype(F32), np.tile(my[:, None], (1, dw)).astype(F32)


CASES["zoom/20x12_to_64x33"] = _zoom(20, 12, 64, 33)
CASES["zoom/64x33_to_20x12"] = _zoom(64, 33, 20, 12)

GROUPS = sorted({k.split("/")[0] for k in CASES})


# ---- calibrations -------------------------------------------------------------------------------------------------------------------------------------------
def _K(f, cx, cy, skew=0.0):
    return [f, skew, cx, 0.0, f, cy, 0.0, 0.0, 1.0]


def _rot_y(deg):
    a = np.deg2rad(deg)
    c, s = float(np.cos(a)), float(np.sin(a))
    return [c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c]


EYE = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
ZERO_D = [0.0] * 5
PINCUSHION = [0.3, 0.0, 1e-3, -1e-3, 0.0]                                  # the strongest the raw-frame tests use (their case C)
BARREL = [-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0]       # (their case B, the right eye)
_K0 = _K(30.0, 19.5, 11.5)     # 40 x 24: the corners are at a normalised radius of 0.76
W0, H0 = 40, 24

# horizon_in_image: 80 degrees about y puts _w = 0 at a column inside the image.  P's principal point and a skew of 2^-30 are chosen so that _w is EXACTLY
# zero at one pixel (NaN), a multiple of the tiny per-row step in the other rows of that column (finite in fp64, beyond fp32: an infinity), and about 0.03 in
# the neighbouring columns (finite, beyond 2^26 with these coefficients).  tests/test_remap_cases.py asserts all three are there.
HORIZON_D = [0.3, 0.5, 1e-3, -1e-3, 0.2]
_C80, _S80 = 0.17364817766693041, 0.984807753012208      # cos, sin of 80 degrees, as literals: the exact zero below depends on their last bit
HORIZON_R = [_C80, 0.0, _S80, 0.0, 1.0, 0.0, -_S80, 0.0, _C80]
HORIZON_P = [30.000015258789062, 2.0 ** -30, 19.28981211214716, 0.0, 30.000015258789062, 11.5, 0.0, 0.0, 1.0]   # f = 30 + 2^-16; cx = 14 + f cos / sin, to the bit

CALIBRATIONS = {
    "identity": (_K0, ZERO_D, EYE, _K0, W0, H0),
    "shift_by_1_5_px": (_K0, ZERO_D, EYE, _K(30.0, 21.0, 13.0), W0, H0),
    "barrel": (_K0, BARREL, EYE, _K0, W0, H0),
    "barrel_2x": (_K0, [2 * d for d in BARREL], EYE, _K0, W0, H0),
    "pincushion": (_K0, PINCUSHION, EYE, _K0, W0, H0),
    "pincushion_2x": (_K0, [2 * d for d in PINCUSHION], EYE, _K0, W0, H0),
    "tangential_only": (_K0, [0.0, 0.0, 0.05, -0.03, 0.0], EYE, _K0, W0, H0),
    "rotated_10deg": (_K0, PINCUSHION, _rot_y(10.0), _K0, W0, H0),
    "rotated_30deg": (_K0, PINCUSHION, _rot_y(30.0), _K0, W0, H0),
    "horizon_in_image": (_K0, HORIZON_D, HORIZON_R, HORIZON_P, W0, H0),
    "singular_P":(_K0, PINCUSHION, EYE, [30.0, 0.0, 19.5, 0.0, 0.0, 11.5, 0.0, 0.0, 1.0], W0, H0),   # det(P R) is exactly 0: ir stays the identity
    "zoom_out_4x": (_K0, PINCUSHION, EYE, _K(7.5, 19.5, 11.5), W0, H0),
    "one_pixel": (_K(30.0, 0.25, 0.5), PINCUSHION, EYE, _K(30.0, 0.0, 0.0), 1, 1),
    "one_row": (_K(50.0, 32.0, 0.25), BARREL, EYE, _K(50.0, 31.5, 0.0), 65, 1),
    "one_column": (_K(50.0, 0.25, 32.0), BARREL, EYE, _K(50.0, 0.0, 31.5), 1, 65),
}
