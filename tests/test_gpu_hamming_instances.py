"""-m gpu: k_hamming_batched through its stage entry, every template instance a launch can reach and every bound inside them, against the exact
reference of hamming_util.py.  The tracker never launches this kernel (it matches through k_candidates / k_hamming_batched_lists), so nothing else in
the suite runs it.  Inputs and the dispatch rule's restatement: case_tables.py; what they are built to reach is asserted without a GPU in
test_case_tables.py.  Every case pre-fills the output with a sentinel and compares all four fields of every query."""
import numpy as np
import pytest

from case_tables import (HAMMING_CHUNKED_GRID, HAMMING_CHUNKED_ROW, HAMMING_COUNT_GEOMETRY, HAMMING_FAMILIES, HAMMING_GEOMETRY, HAMMING_INSTANCE_CASES,
                         HAMMING_PACKED_LAYOUTS, HAMMING_R2_BOUNDARIES, HB_MMAX, HB_NMAX, hamming_admitted, hamming_boundary_problem,
                         hamming_chunked_grid_case, hamming_chunked_row_case, hamming_count_case, hamming_count_check, hamming_instance,
                         hamming_instance_problem, hamming_packed_starts_case, hamming_phantom_case, hamming_scan_chunk, hamming_nbins)
from hamming_util import NO_NEIGHBOUR, hamming_ref, mismatches

pytestmark = pytest.mark.gpu

SENTINEL = -77


def _run(hip_lib, qd, qxy, td, txy, tf, r2, mode, rows, cols):
    """the entry on device copies of one batch; returns the (B, M, 4) records, every word of which the kernel must have written"""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    B, M = qd.shape[:2]
    out = torch.full((B, M, 4), SENTINEL, dtype=torch.int32, device="cuda")
    us = hip_lib.hamming_match_batched(t(qd), t(qxy), t(td), t(txy), t(tf), float(r2), mode, rows, cols, out)
    assert us > 0 or td.shape[1] == 0
    return out.cpu().numpy()


def _hold(hip_lib, qd, qxy, td, txy, tf, r2, mode, rows, cols, tag=""):
    ref = hamming_ref(qd, qxy, td, txy, tf, r2, mode, rows)
    got = _run(hip_lib, qd, qxy, td, txy, tf, r2, mode, rows, cols)
    assert np.array_equal(got, ref), f"{tag}: {mismatches(got, ref)}"
    return ref


@pytest.mark.parametrize("fam,q,t,member,M,N", HAMMING_INSTANCE_CASES, ids=[f"{c[0]}-q{c[1]}t{c[2]}-{c[3]}" for c in HAMMING_INSTANCE_CASES])
def test_every_instance(hip_lib, fam, q, t, member, M, N):
    """<MODE, NSP, QPT, TPT> for the four families x the fifteen (QPT, TPT) classes the LDS admits, at the smallest and the largest member of each
    class (the largest sits at the LDS bound where the class reaches it).  Problem 0: uniform features, flags, descriptor ties, queries outside the
    image; problem 1: a dense cluster (windows past 64 candidates, ranges past 63) and, in row mode, rows that send the walk to its comparison."""
    mode, nsp, r2 = HAMMING_FAMILIES[fam]
    rows, cols = HAMMING_GEOMETRY
    assert hamming_instance(mode, r2, M, N) == (mode, nsp, q, t)
    qd, qxy, td, txy, tf = hamming_instance_problem(fam, M, N)
    ref = _hold(hip_lib, qd, qxy, td, txy, tf, r2, mode, rows, cols, f"{fam} M={M} N={N}")
    if member == "largest":
        assert (ref[:, :, 2] >= 0).mean() > 0.3 and (ref[:, :, 0] < 0).any()       # records of both kinds were compared


@pytest.mark.parametrize("csr", [1, 2], ids=["r2_625_packed", "r2_2500_two_stage"])
def test_candidate_count_bounds(hip_lib, csr):
    """populations with exactly k = 31, 32, 33, 40, 41, 42, 63, 64, 65 (66) window candidates, all in one range and split over the ranges (a single range
    of 63 and of 64): either side of the lo | hi mask words, of MASK_BITS = 41, of the 6-bit range length and of the two-word mask's 64.  About half of
    each population lies inside the circle, some of it at distance^2 == r2; every feature has a query carrying its descriptor."""
    rows, cols = HAMMING_COUNT_GEOMETRY
    hamming_count_check(csr)                      # the counts are what they are meant to be: binned on the CPU, range by range
    qd, qxy, td, txy, tf, pops = hamming_count_case(csr)
    r2 = 625.0 * csr * csr
    assert hamming_instance(0, r2, qd.shape[1], td.shape[1]) == (0, 3 if csr == 1 else 5, 1, 1)
    ref = _hold(hip_lib, qd, qxy, td, txy, tf, r2, 0, rows, cols, f"csr {csr}")
    assert (ref[:, :, 1] == 1).mean() > 0.3       # the planted queries found their features one bit away


@pytest.mark.parametrize("r2,fam", HAMMING_R2_BOUNDARIES, ids=[f"r2_{float(r):.9g}" for r, _ in HAMMING_R2_BOUNDARIES])
def test_dispatch_boundaries_in_r2(hip_lib, r2, fam):
    """r2 = 0, 1e-3, 625 | its fp32 successor (csr 1 -> 2), 2500 | its successor (csr 2 -> any csr), 40000: train features at distance 0, 25 and 50
    exactly from sixty queries keep the radius decision on the boundary while the family switches"""
    rows, cols = HAMMING_GEOMETRY
    qd, qxy, td, txy, tf = hamming_boundary_problem()
    assert hamming_instance(0, r2, qd.shape[1], td.shape[1])[:2] == HAMMING_FAMILIES[fam][:2]
    ref = _hold(hip_lib, qd, qxy, td, txy, tf, r2, 0, rows, cols, f"r2 {float(r2)!r}")
    if r2 == 0:
        assert (ref == np.array(NO_NEIGHBOUR * 2, np.int32)).all()


_CHUNKED = [(1, rows, None, 0.0) for rows in HAMMING_CHUNKED_ROW] + [(0, rows, cols, r2) for rows, cols, r2 in HAMMING_CHUNKED_GRID]


@pytest.mark.parametrize("mode,rows,cols,r2", _CHUNKED, ids=[f"rows_{r}" if m else f"grid_{c}x{r}-r2_{int(r2)}" for m, r, c, r2 in _CHUNKED])
def test_chunked_bin_scan(hip_lib, mode, rows, cols, r2):
    """the bin scan with more entries than threads.  Row mode at 1022 (the last height on the one-entry-per-thread arm), 1023, 1024 and 2160 image rows:
    features on the first and last rows, on row `rows` itself and in every chunk of the scan, queries at both borders.  Radius mode on 164 x 48 and
    104 x 40 hash cells (7 873 and 4 161 entries, neither a multiple of the per-thread chunk) in all three radius families: a feature in every chunk,
    windows on the last cell column and row and across the wrap between cell rows."""
    if mode == 1:
        qd, qxy, td, txy, tf, cols = hamming_chunked_row_case(rows)
        assert (hamming_scan_chunk(hamming_nbins(1, rows, cols)) > 0) == (rows >= 1023)
    else:
        qd, qxy, td, txy, tf = hamming_chunked_grid_case(rows, cols)
        assert hamming_scan_chunk(hamming_nbins(0, rows, cols)) > 1
    ref = _hold(hip_lib, qd, qxy, td, txy, tf, r2, mode, rows, cols, f"{cols} x {rows}")
    assert (ref[:, :, 0] >= 0).mean() > 0.3


@pytest.mark.parametrize("layout", HAMMING_PACKED_LAYOUTS)
def test_packed_starts_at_2048(hip_lib, layout):
    """N = 2048 without a flag: the start of a range behind the last populated cell IS 2048 and does not fit the 11-bit field of the packed slot words.
    All three starts (`behind`), the two behind a first range of even and of odd length (`tail`), and the same at N = 2047 (`control`)."""
    rows, cols = HAMMING_GEOMETRY
    qd, qxy, td, txy, tf = hamming_packed_starts_case(layout)
    _hold(hip_lib, qd, qxy, td, txy, tf, 625.0, 0, rows, cols, layout)


def test_packed_start_overflow_changes_no_record(hip_lib):
    """the constructed input of hamming_phantom_case: unguarded, the overflow of the start fields makes query Q test the slot words of query 0 as a train
    feature's coordinates, and they decode to a point 4 px from Q -- whose record must stay `no neighbour`"""
    rows, cols = HAMMING_GEOMETRY
    qd, qxy, td, txy, tf, info = hamming_phantom_case()
    ref = _hold(hip_lib, qd, qxy, td, txy, tf, 625.0, 0, rows, cols, "phantom")
    assert ref[0, info["Q"]].tolist() == list(NO_NEIGHBOUR * 2) and (ref[0, info["heavy"], 2] >= 0).all()


def test_refused_sizes(hip_lib):
    """sizes the entry refuses WITHOUT launching: (3073, 3073) and one feature past the largest member of a class (more LDS than a workgroup has), N = 4097
    and M = 4097 (the caps).  The wrapper raises, the output keeps its sentinel, and an ordinary call behind each refusal is exact."""
    import torch
    rows, cols = HAMMING_GEOMETRY
    rng = np.random.default_rng(9)
    fam, q, t, member, M1, N1 = next(c for c in HAMMING_INSTANCE_CASES if c[:4] == ("csr1", 1, 4, "largest"))
    sizes = [(3073, 3073, (0, 1)), (M1, N1 + 1, (0,)), (8, HB_NMAX + 1, (0, 1)), (HB_MMAX + 1, 8, (0, 1))]
    small = hamming_instance_problem("csr1", 1, 1025)
    for M, N, modes in sizes:
        for mode in (0, 1):
            assert hamming_admitted(mode, M, N, rows, cols) == (mode not in modes)
        qd = torch.from_numpy(rng.integers(0, 256, (1, M, 32), dtype=np.uint8)).cuda()
        td = torch.from_numpy(rng.integers(0, 256, (1, N, 32), dtype=np.uint8)).cuda()
        qxy = torch.from_numpy((rng.uniform(0, 1, (1, M, 2)) * [cols - 1, rows - 1]).astype(np.float32)).cuda()
        txy = torch.from_numpy(np.floor(rng.uniform(0, 1, (1, N, 2)) * [cols - 1, rows - 1]).astype(np.float32)).cuda()
        tf = torch.zeros((1, N), dtype=torch.uint8, device="cuda")
        out = torch.full((1, M, 4), SENTINEL, dtype=torch.int32, device="cuda")
        for mode, r2 in ((0, 625.0), (1, 0.0)):
            if mode not in modes:
                continue
            with pytest.raises(RuntimeError):
                hip_lib.hamming_match_batched(qd, qxy, td, txy, tf, r2, mode, rows, cols, out)
            torch.cuda.synchronize()
            assert bool((out == SENTINEL).all()), (M, N, mode)
        _hold(hip_lib, *small, 625.0, 0, rows, cols, f"after ({M}, {N})")


def test_no_train_features_at_three_queries_per_thread(hip_lib):
    """N = 0 with M = 3000: k_hamming_none writes `no neighbour` for every query of every problem, and nothing else"""
    import torch
    rows, cols = HAMMING_GEOMETRY
    B, M = 3, 3000
    rng = np.random.default_rng(3000)
    qd = torch.from_numpy(rng.integers(0, 256, (B, M, 32), dtype=np.uint8)).cuda()
    qxy = torch.from_numpy((rng.uniform(0, 1, (B, M, 2)) * [cols - 1, rows - 1]).astype(np.float32)).cuda()
    empty = lambda *shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    for mode in (0, 1):
        out = torch.full((B * M + 64, 4), SENTINEL, dtype=torch.int32, device="cuda")      # 64 records of slack behind the batch: they keep the sentinel
        us = hip_lib.hamming_match_batched(qd, qxy, empty(B, 0, 32, dt=torch.uint8), empty(B, 0, 2, dt=torch.float32), empty(B, 0, dt=torch.uint8),
                                           625.0, mode, rows, cols, out)
        got = out.cpu().numpy()
        assert us == 0.0 and (got[:B * M] == np.array(NO_NEIGHBOUR * 2, np.int32)).all() and (got[B * M:] == SENTINEL).all()
