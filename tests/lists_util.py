"""The candidate lists of the tracker, restated in plain numpy (lvt_image_features_struct.cpp:68-148 without the marks): per query the train features that pass
the window predicate, as keys  popcount(query ^ train) << 16 | train index  in ascending order, and their full count.  Both predicates are evaluated in fp32
with one rounding per written operation (numpy does not fuse a multiply into an add), which is what the reference computes; everything that comes out is an
integer, so the comparison with a builder's list (`hold`) is equality.

The map / staged references take the device's OWN projections and visibility (lvt_amd_get_candidate_lists) as queries: the list stage is then exact given its
input, and the projection is held elsewhere (test_gpu_parity.py).  The row reference takes the two feature sets."""
import numpy as np

KC = 128            # list capacity (lvt_dev.h)
HASH_CELL = 25      # px (lvt_image_features_struct.cpp:48)
ROW_RADIUS = 2      # rows (lvt_image_features_struct.cpp:124-131)
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint16)
f32 = np.float32


def cell_search_radius(radius):
    """lvt_image_features_struct.cpp:50-53"""
    return 1 if radius == HASH_CELL else int(np.ceil(f32(radius) / f32(HASH_CELL)))


def hash_grid(width, height):
    return int(np.ceil(width / float(HASH_CELL))), int(np.ceil(height / float(HASH_CELL)))


def hash_cells(xy):
    """floor(x / 25.f), floor(y / 25.f) in fp32: the cell a feature is filed under and the cell a query's window is centred on"""
    xy = np.asarray(xy, f32).reshape(-1, 2)
    return np.floor(xy / f32(HASH_CELL)).astype(np.int64)


def row_mask(xy_left, xy_right, height):
    """[n_left, n_right] bool: the row-matching predicate.  The band is int(y) +- 2 clipped to [0, H]; a train feature is inside when
    y_r >= lo and y_r <= hi, compared as floats (struct.cpp:124-134)"""
    yl = np.asarray(xy_left, f32).reshape(-1, 2)[:, 1]
    yr = np.asarray(xy_right, f32).reshape(-1, 2)[:, 1]
    lo = np.maximum(yl.astype(np.int64) - ROW_RADIUS, 0).astype(f32)       # int(): truncation
    hi = np.minimum(yl.astype(np.int64) + ROW_RADIUS, height).astype(f32)
    return (yr[None, :] >= lo[:, None]) & (yr[None, :] <= hi[:, None])


def track_window(proj, radius, width, height):
    """[n, 4] the queries' cell windows (sx, ex, sy, ey), half open, clipped to the grid (struct.cpp:76-88).  The window follows the TRACKING radius: the second
    pass doubles the radius of the distance test only"""
    ccx, ccy = hash_grid(width, height)
    csr = cell_search_radius(radius)
    h = hash_cells(proj)
    return np.column_stack([np.maximum(h[:, 0] - csr, 0), np.minimum(h[:, 0] + csr + 1, ccx), np.maximum(h[:, 1] - csr, 0), np.minimum(h[:, 1] + csr + 1, ccy)])


def track_d2(proj, xy):
    """[n, N] fp32: dx * dx + dy * dy with dx = x_feature - x_query, each operation rounded once"""
    p = np.asarray(proj, f32).reshape(-1, 2)
    t = np.asarray(xy, f32).reshape(-1, 2)
    dx = t[None, :, 0] - p[:, None, 0]
    dy = t[None, :, 1] - p[:, None, 1]
    return dx * dx + dy * dy


def track_masks(proj, vis, xy, radius, width, height, pass2=False):
    """(in the window's cells, and inside the radius too), both [n, N] bool: the tracking predicate (struct.cpp:76-99).  r2 = radius^2, (2 radius)^2 for the
    second pass; an invisible point has no candidates"""
    w = track_window(proj, radius, width, height)
    c = hash_cells(xy)
    cells = (c[None, :, 0] >= w[:, None, 0]) & (c[None, :, 0] < w[:, None, 1]) & (c[None, :, 1] >= w[:, None, 2]) & (c[None, :, 1] < w[:, None, 3])
    cells &= np.asarray(vis).astype(bool)[:, None]
    r = radius * (2 if pass2 else 1)
    d2 = track_d2(proj, xy)
    assert d2.dtype == np.float32
    return cells, cells & (d2 < f32(r * r))


def lists_from_mask(q_desc, t_desc, mask):
    """keys [n, KC] uint32 (0xFFFFFFFF past a list's end) and counts [n]: the masked train features of every query by (distance, index).  The popcounts are
    taken of the masked pairs only, so 4096 x 4096 features stay cheap"""
    q_desc = np.asarray(q_desc, np.uint8).reshape(-1, 32)
    t_desc = np.asarray(t_desc, np.uint8).reshape(-1, 32)
    n = len(q_desc)
    keys = np.full((n, KC), 0xFFFFFFFF, np.uint32)
    counts = np.zeros(n, np.int32)
    full = []
    for q in range(n):
        idx = np.flatnonzero(mask[q])
        counts[q] = len(idx)
        d = _POP[q_desc[q][None, :] ^ t_desc[idx]].sum(axis=1).astype(np.uint32)
        k = np.sort((d << np.uint32(16)) | idx.astype(np.uint32))
        full.append(k)
        keys[q, :min(len(k), KC)] = k[:KC]
    return keys, counts, full


def row_lists(xy_left, desc_left, xy_right, desc_right, height):
    m = row_mask(xy_left, xy_right, height)
    keys, counts, full = lists_from_mask(desc_left, desc_right, m)
    return {"keys": keys, "counts": counts, "full": full, "mask": m}


def track_lists(proj, vis, q_desc, xy, desc, radius, width, height, pass2=False):
    cells, m = track_masks(proj, vis, xy, radius, width, height, pass2)
    keys, counts, full = lists_from_mask(q_desc, desc, m)
    return {"keys": keys, "counts": counts, "full": full, "mask": m, "cells": cells}


def equal_distance_neighbours(full):
    """adjacent entries of equal distance over all lists: where the index decides the order"""
    return int(sum(((k[1:] >> 16) == (k[:-1] >> 16)).sum() for k in full if len(k) > 1))


def hold(got, ref, tag, vis=None):
    """a builder's lists against the reference's, query by query: the counts everywhere; the keys [0, n) where n <= KC (beyond min(n, KC) a list is
    unspecified, and above KC only the count holds); no candidates for an invisible point.  Prints the first differing query and position."""
    gk, gn = np.asarray(got["keys"]), np.asarray(got["counts"])
    rk, rn = np.asarray(ref["keys"]), np.asarray(ref["counts"])
    assert len(gn) == len(rn), f"{tag}: {len(gn)} lists, the reference has {len(rn)}"
    bad = np.flatnonzero(gn != rn)
    if bad.size:
        q = int(bad[0])
        print(f"{tag}: first differing count at query {q}: got {int(gn[q])}, reference {int(rn[q])} ({bad.size} counts differ)")
    assert bad.size == 0, (tag, "counts", bad[:8], gn[bad[:8]], rn[bad[:8]])
    if vis is not None:
        assert (gn[~np.asarray(vis).astype(bool)] == 0).all(), (tag, "an invisible point has candidates")
    held = 0
    for q in np.flatnonzero((rn > 0) & (rn <= KC)):
        n = int(rn[q])
        if not np.array_equal(gk[q, :n], rk[q, :n]):
            p = int(np.flatnonzero(gk[q, :n] != rk[q, :n])[0])
            print(f"{tag}: first differing list: query {q} (n = {n}), position {p}: got {int(gk[q, p]):#x}, reference {int(rk[q, p]):#x}")
            raise AssertionError((tag, "keys", int(q), p, gk[q, :n].tolist(), rk[q, :n].tolist()))
        held += n
    return held
