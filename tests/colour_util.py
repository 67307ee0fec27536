"""Colour inputs for the pixel-format tests, and the numpy restatement of the conversion they are held to.  Nothing here comes from the library under test:
the formula is the one include/lvt_amd_ext.h documents (cv::cvtColor's 8-bit BGR2GRAY), restated on integers."""
import numpy as np

GRAY8, BGR8, RGB8, BGRA8, RGBA8 = 0, 1, 2, 3, 4
BPP = {GRAY8: 1, BGR8: 3, RGB8: 3, BGRA8: 4, RGBA8: 4}
COLOUR_FORMATS = (BGR8, RGB8, BGRA8, RGBA8)
NAMES = {GRAY8: "GRAY8", BGR8: "BGR8", RGB8: "RGB8", BGRA8: "BGRA8", RGBA8: "RGBA8"}
KNOWN_ANSWERS = [((255, 0, 0), 76), ((0, 255, 0), 150), ((0, 0, 255), 29), ((255, 255, 255), 255)]   # (R, G, B) -> gray


def channel_offsets(fmt):
    """byte offsets of (R, G, B) inside a pixel of the format"""
    return (2, 1, 0) if fmt in (BGR8, BGRA8) else (0, 1, 2)


def gray_of_rgb(r, g, b):
    """gray = (R 4899 + G 9617 + B 1868 + 8192) >> 14 on integer arrays (or scalars)"""
    r, g, b = (np.asarray(x).astype(np.int64) for x in (r, g, b))
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def to_gray(img, fmt):
    """(H, W, bpp) uint8 in `fmt` -> (H, W) uint8"""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == BPP[fmt], (img.shape, fmt)
    ro, go, bo = channel_offsets(fmt)
    return np.ascontiguousarray(gray_of_rgb(img[:, :, ro], img[:, :, go], img[:, :, bo]))


def pack(r, g, b, alpha, fmt):
    """interleave the channels in the format's order; alpha is used by the 4-byte formats only"""
    H, W = r.shape
    out = np.empty((H, W, BPP[fmt]), np.uint8)
    ro, go, bo = channel_offsets(fmt)
    out[:, :, ro], out[:, :, go], out[:, :, bo] = r, g, b
    if BPP[fmt] == 4:
        out[:, :, 3] = alpha
    return out


def colour_channels(gray, world, frame, eye):
    """(R, G, B, alpha) of a gray rendering: every channel is clip(g + d) with independent integer noise, d in [-24, 24] for R, [-8, 8] for G, [-32, 32]
    for B; alpha is random bytes.  The amplitudes differ per channel: a swapped channel order or a used alpha byte changes most gray pixels.  The draw does
    not depend on the format, so every format of a frame converts to the same gray image."""
    rng = np.random.default_rng([int(world), int(frame), int(eye)])
    g = gray.astype(np.int64)
    ch = [np.clip(g + rng.integers(-a, a + 1, size=g.shape), 0, 255).astype(np.uint8) for a in (24, 8, 32)]
    alpha = rng.integers(0, 256, size=g.shape, dtype=np.uint8)
    return ch[0], ch[1], ch[2], alpha


def colourise(gray, fmt, world, frame, eye):
    return pack(*colour_channels(gray, world, frame, eye), fmt)
