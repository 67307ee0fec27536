"""CPU tier: the cheap exact reference of the batched Hamming matcher (hamming_util.py) is held to the oracle's own top-2 on small problems, and to the
earlier (M, N, 32)-table helper of test_gpu_primitives.py at one mid size -- before the GPU tier uses it at sizes neither of them reaches."""
import numpy as np
import pytest

from hamming_util import NO_NEIGHBOUR, bit_distances, hamming_ref, problem_mask, records_from_distances


def _problem(rng, B, M, N, rows, cols, variant):
    td = rng.integers(0, 256, (B, N, 32), dtype=np.uint8)
    qd = rng.integers(0, 256, (B, M, 32), dtype=np.uint8)
    if variant == "ties":             # 4 prototypes: most distances tie, many at 0
        proto = rng.integers(0, 256, (4, 32), dtype=np.uint8)
        td, qd = proto[rng.integers(0, 4, (B, N))], proto[rng.integers(0, 4, (B, M))]
    txy = np.floor(rng.uniform(0, 1, (B, N, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    qxy = (rng.uniform(0, 1, (B, M, 2)) * [cols - 1, rows - 1]).astype(np.float32)
    tf = (rng.uniform(0, 1, (B, N)) < 0.2).astype(np.uint8)
    if variant == "all_masked":
        tf[:] = 1
    if variant == "single":           # one candidate per query at most: every feature flagged but one, which sits on query 0
        tf[:] = 1
        tf[:, N // 2] = 0
        txy[:, N // 2] = np.floor(qxy[:, 0])
    if variant == "rows":             # fractional, out-of-range and NaN train rows, queries at both borders
        txy[:, ::3, 1] += np.float32(0.5)
        txy[:, 1, 1], txy[:, 2, 1], txy[:, 4, 1], txy[:, 5, 1] = np.float32(np.nan), np.float32(-3.0), np.float32(rows), np.float32(rows + 2.5)
        qxy[:, :4, 1] = np.array([0.0, 1.9, rows - 0.5, rows + 2.0], np.float32)
    return qd, qxy, td, txy, tf


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("variant", ["random", "ties", "all_masked", "single", "rows"])
def test_reference_equals_the_oracle(oracle_lib, mode, variant):
    """every record of small problems against lvto_hamming_top2 under the same masks: distances, the (distance, index) order, the no-neighbour record"""
    rng = np.random.default_rng([mode, len(variant)])
    B, M, N, rows, cols = 3, 40, 90, 120, 200                 # dense enough for several candidates per query in either mode
    r2 = 2500.0
    qd, qxy, td, txy, tf = _problem(rng, B, M, N, rows, cols, variant)
    got = hamming_ref(qd, qxy, td, txy, tf, r2, mode, rows)
    assert got.dtype == np.int32 and got.shape == (B, M, 4)
    n_two = 0
    for b in range(B):
        mask = problem_mask(qxy[b], txy[b], tf[b], r2, mode, rows).astype(np.uint8)
        for m in range(M):
            assert tuple(got[b, m]) == oracle_lib.hamming_top2(qd[b, m], td[b], mask[m]), (b, m)
            n_two += int(mask[m].sum() >= 2)
    if variant in ("random", "ties", "rows"):
        assert n_two >= B * M // 3                             # the order is decided among several candidates, not by default
    if variant == "all_masked":
        assert (got == np.array(NO_NEIGHBOUR * 2, np.int32)).all()
    if variant == "single":
        assert (got[:, :, 2:] == np.array(NO_NEIGHBOUR, np.int32)).all() and (got[:, 0, 0] == N // 2).all()
    if variant == "ties":
        tie = (got[:, :, 1] == got[:, :, 3]) & (got[:, :, 2] >= 0)
        assert tie.sum() >= 20 and (got[:, :, 0] < got[:, :, 2])[tie].all()      # (ties exist in both modes, and go to the lowest index)


def test_bit_matrix_distances_are_popcounts():
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 256, (70, 32), dtype=np.uint8), rng.integers(0, 256, (130, 32), dtype=np.uint8)
    a[0], b[0], a[1], b[1] = 0, 255, 255, 255                # distance 256 and 0
    pop = np.array([bin(i).count("1") for i in range(256)], np.int32)
    d = bit_distances(a, b)
    assert d.dtype == np.int32 and np.array_equal(d, pop[a[:, None, :] ^ b[None, :, :]].sum(axis=2))
    assert d[0, 0] == 256 and d[1, 1] == 0
    # no train feature at all, and a single one: the record still has its "second"
    assert (records_from_distances(np.zeros((3, 0), np.int32), np.zeros((3, 0), bool)) == np.array(NO_NEIGHBOUR * 2, np.int32)).all()
    assert records_from_distances(np.array([[7]]), np.array([[True]])).tolist() == [[0, 7, *NO_NEIGHBOUR]]


@pytest.mark.parametrize("mode,r2", [(0, 625.0), (0, 5625.0), (1, 0.0)])
def test_reference_equals_the_table_helper_at_a_mid_size(mode, r2):
    """(M, N) = (300, 700) on 1241 x 376 with a dense cluster, prototypes, flags and queries outside the image: the (M, N, 32)-table helper the
    existing GPU tests use and the bit-matrix reference give the same records"""
    from test_gpu_primitives import _hamming_ref_np
    rng = np.random.default_rng(300 + mode)
    B, M, N, rows, cols = 2, 300, 700, 376, 1241
    qd, qxy, td, txy, tf = _problem(rng, B, M, N, rows, cols, "random")
    proto = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    td[1], qd[1] = proto[rng.integers(0, 8, N)], proto[rng.integers(0, 8, M)]
    txy[0, :N // 2] = np.floor(rng.uniform(0, 1, (N // 2, 2)) * [120, 90] + [300, 100]).astype(np.float32)
    qxy[0, :M // 2] = (rng.uniform(0, 1, (M // 2, 2)) * [120, 90] + [300, 100]).astype(np.float32)
    qxy[1, :10] = rng.uniform(-60, 0, (10, 2)).astype(np.float32)
    qxy[1, 10:20] += np.float32(1300)
    if mode == 1:
        txy[0, ::5, 1] += np.float32(0.25)
        txy[0, 3, 1] = np.float32(np.nan)
    a = hamming_ref(qd, qxy, td, txy, tf, r2, mode, rows)
    b = _hamming_ref_np(qd, qxy, td, txy, tf, r2, mode, rows)
    assert np.array_equal(a, b)
    assert (a[:, :, 0] >= 0).mean() > 0.5 and (a[:, :, 0] < 0).any()
