"""The semantics of the batched masked 2-NN Hamming matcher (cv::BFMatcher::knnMatch(k = 2, mask) behind lvt_image_features_struct.cpp:68-148), stated
once for the tests: the two fp32 masks, the record format, and an exact reference that is cheap at M, N in the thousands.  Nothing here needs a GPU.

A problem is (qd (M, 32) u8, qxy (M, 2) f32, td (N, 32) u8, txy (N, 2) f32, tf (N,) u8); a batch stacks B of them on a leading axis.  The record of a
query is (idx1, d1, idx2, d2): its two nearest unmasked, unflagged train features by (distance, index), NO_NEIGHBOUR where there is none."""
import numpy as np

NO_NEIGHBOUR = (-1, 0x7FFFFFFF)
ROW_RADIUS = 2
_MASKED = np.int32(1 << 30)          # above every key: a key is distance * 65536 + index < 257 * 65536


def radius_mask(qxy, txy, r2):
    """(M, N) bool: (dx * dx + dy * dy) < r2 with every step rounded to fp32 (struct.cpp:95-99); strict, NaN fails"""
    dx = (txy[None, :, 0] - qxy[:, None, 0]).astype(np.float32)
    dy = (txy[None, :, 1] - qxy[:, None, 1]).astype(np.float32)
    return ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32) < np.float32(r2)


def row_mask(qxy, txy, rows):
    """(M, N) bool: ty >= max(int(y) - 2, 0) and ty <= min(int(y) + 2, rows) (struct.cpp:124-133); a NaN train row fails both comparisons"""
    y = qxy[:, 1]
    s = np.maximum(y.astype(np.int64) - ROW_RADIUS, 0)[:, None]
    e = np.minimum(y.astype(np.int64) + ROW_RADIUS, rows)[:, None]
    ty = txy[None, :, 1]
    return (ty >= s) & (ty <= e)


def problem_mask(qxy, txy, tf, r2, mode, rows):
    """the candidates of every query: the mode's mask, flagged train features excluded"""
    mask = radius_mask(qxy, txy, r2) if mode == 0 else row_mask(qxy, txy, rows)
    return mask & (tf == 0)[None, :]


def records_from_distances(d, mask):
    """(M, 4) int32 records from an (M, N) table of integer distances and the (M, N) candidate mask: top-2 by (distance, index)"""
    M, N = d.shape
    assert N < 65536
    out = np.empty((M, 4), np.int32)
    out[:, 0::2], out[:, 1::2] = NO_NEIGHBOUR
    if N == 0 or M == 0:
        return out
    key = np.where(mask, d.astype(np.int32) * np.int32(65536) + np.arange(N, dtype=np.int32)[None, :], _MASKED)
    rows = np.arange(M)
    for k in (0, 1):
        j = np.argmin(key, axis=1)                    # keys of unmasked entries are distinct: the minimum is the (distance, index) order's
        kk = key[rows, j]
        has = kk < _MASKED
        out[has, 2 * k] = kk[has] & 0xFFFF
        out[has, 2 * k + 1] = kk[has] >> 16
        key[rows, j] = _MASKED
    return out


def bit_distances(qd, td):
    """(M, N) Hamming distances of 256-bit descriptors as a bit-matrix product: with a, b the 0 / 1 matrices of the bits,
    d = a (1 - b)^T + (1 - a) b^T.  Every partial sum is an integer <= 256 < 2^24: exact in fp32 whatever the summation order."""
    a = np.unpackbits(np.ascontiguousarray(qd, np.uint8).reshape(len(qd), 32), axis=1).astype(np.float32)
    b = np.unpackbits(np.ascontiguousarray(td, np.uint8).reshape(len(td), 32), axis=1).astype(np.float32)
    d = a @ (np.float32(1) - b).T + (np.float32(1) - a) @ b.T
    return d.astype(np.int32)


def hamming_ref_problem(qd, qxy, td, txy, tf, r2, mode, rows):
    """(M, 4) records of ONE problem"""
    if len(td) == 0:
        return records_from_distances(np.zeros((len(qd), 0), np.int32), np.zeros((len(qd), 0), bool))
    return records_from_distances(bit_distances(qd, td), problem_mask(qxy, txy, tf, r2, mode, rows))


def hamming_ref(qd, qxy, td, txy, tf, r2, mode, rows):
    """(B, M, 4) records of a batch"""
    return np.stack([hamming_ref_problem(qd[b], qxy[b], td[b], txy[b], tf[b], r2, mode, rows) for b in range(len(qd))])


def mismatches(got, ref):
    """a readable account of the first queries whose records differ ('' when none does)"""
    bad = np.argwhere((got != ref).any(axis=-1))
    if bad.size == 0:
        return ""
    first = tuple(bad[0])
    return f"{len(bad)} queries differ, first {bad[:3].tolist()}: got {got[first].tolist()} ref {ref[first].tolist()}"
