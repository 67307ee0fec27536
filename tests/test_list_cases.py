"""CPU tier of the candidate-list tests: the reference of tests/lists_util.py against the oracle, and the planted cases of tests/list_cases.py against
what they claim -- with the oracle alone, before tests/test_gpu_candidate_lists.py holds the device's list builders to them.

Row cases: the oracle tracks the case's one frame; the reference lists over ITS features must plant what the case claims (band membership at the fp32
edges, window totals, capacities, counts, equal-distance neighbours), and the first two entries of every list must be lvto_hamming_top2's under the reference's
own mask.  Map cases: the oracle tracks the three frames; the nominal projections of its map (a static camera: the identity pose) stand in for the
device's, and the reference over them must show the exact-radius pairs, the clipped windows, the window totals and list lengths the case claims."""
import numpy as np
import pytest

import list_cases as LC
from hamming_util import NO_NEIGHBOUR
import lists_util as LU


def _oracle_frames(oracle_lib, case, upto):
    orc = oracle_lib.Oracle(case["prm"], 1)
    for f in case["frames"][:upto]:
        orc.track_with_external_corners(*f)
    return orc


def _top2_of(full_q):
    rec = list(NO_NEIGHBOUR * 2)
    for k, key in enumerate(full_q[:2]):
        rec[2 * k], rec[2 * k + 1] = int(key & 0xFFFF), int(key >> 16)
    return tuple(rec)


@pytest.mark.parametrize("name", sorted(LC.ROW_CASES))
def test_row_case_plants_what_it_claims(oracle_lib, name):
    case = LC.ROW_CASES[name]()
    orc = _oracle_frames(oracle_lib, case, 1)
    (xl, _, dl), (xr, _, dr) = orc.features(0), orc.features(1)
    ref = LU.row_lists(xl, dl, xr, dr, case["H"])
    LC.check_row_claims(case, xl, xr, ref)
    step = max(1, len(xl) // 300)                                   # (every list of the small cases, every 13th of 4096)
    for q in range(0, len(xl), step):
        want = oracle_lib.hamming_top2(dl[q], dr, ref["mask"][q].astype(np.uint8)) if len(xr) else NO_NEIGHBOUR * 2
        got = _top2_of(ref["full"][q])
        assert got == tuple(want), (name, q, got, want)
    # the stand-down sizes: what the binned kernel's switch reads
    assert case["expect"]["stood_down_row"] == int(len(xr) > LC.LS_NMAX or case["H"] + 1 > LC.LS_BINS)


@pytest.mark.parametrize("name", sorted(LC.MAP_CASES))
def test_map_case_plants_what_it_claims(oracle_lib, name):
    case = LC.MAP_CASES[name]()
    c = case["claims"]
    staged = c.get("staged", False)
    orc = _oracle_frames(oracle_lib, case, 1)
    assert orc.counts()["map_size"] == c["n0"], (orc.counts(), c["n0"])            # every corner of frame 0 was triangulated: the early count
    orc.track_with_external_corners(*case["frames"][1])
    xyz, _, _, mdesc = orc.map()
    sxyz, _, sdesc = orc.staged()
    assert (len(xyz), len(sxyz)) == ((c["n0"], c["n1"]) if staged else (c["n0"] + c["n1"], 0)), (len(xyz), len(sxyz))
    orc.track_with_external_corners(*case["frames"][2])
    cnt = orc.counts()
    assert orc.status == 2 and cnt["map_size_at_match"] == len(xyz) and cnt["second_pass"] == case["expect"]["pass2"], cnt
    xy, _, desc = orc.features(0)
    W, H, radius = case["W"], case["H"], case["radius"]
    for which, X, qd in (("map", xyz, mdesc),) + ((("staged", sxyz, sdesc),) if staged else ()):
        proj = LC.nominal_projection(case["prm"], X)
        vis = np.ones(len(proj), np.int8)
        ref = LU.track_lists(proj, vis, qd, xy, desc, radius, W, H, pass2=bool(case["expect"]["pass2"]))
        LC.check_map_claims(case, proj, vis, xy, ref, n_early=c["n0"], which=which)
        for q in range(0, len(proj), max(1, len(proj) // 100)):
            want = oracle_lib.hamming_top2(qd[q], desc, ref["mask"][q].astype(np.uint8))
            got = _top2_of(ref["full"][q])
            assert got == tuple(want), (name, which, q, got, want)
    # the stand-down sizes
    ccx, ccy = LU.hash_grid(W, H)
    assert case["expect"]["stood_down_map"] == int(len(xy) > LC.LS_NMAX or ccx * ccy > LC.LS_BINS or LU.cell_search_radius(radius) > 2)


def test_hold_reports_a_wrong_list():
    """the comparison itself: a swapped pair, a wrong count and a candidate on an invisible point are caught; entries beyond min(n, KC) are not compared"""
    ref = {"keys": np.full((3, LU.KC), 0xFFFFFFFF, np.uint32), "counts": np.array([2, 0, 200], np.int32)}
    ref["keys"][0, :2] = [5 << 16 | 1, 5 << 16 | 3]
    got = {"keys": ref["keys"].copy(), "counts": ref["counts"].copy()}
    got["keys"][0, 2:] = 7                                          # unspecified words
    got["keys"][2] = 9                                              # n > KC: only the count holds
    assert LU.hold(got, ref, "same", vis=np.array([1, 0, 1])) == 2
    swapped = {"keys": got["keys"].copy(), "counts": got["counts"]}
    swapped["keys"][0, :2] = swapped["keys"][0, 1::-1]
    with pytest.raises(AssertionError):
        LU.hold(swapped, ref, "swapped")
    with pytest.raises(AssertionError):
        LU.hold({"keys": got["keys"], "counts": np.array([2, 0, 129], np.int32)}, ref, "count")
    with pytest.raises(AssertionError):
        LU.hold({"keys": got["keys"], "counts": np.array([2, 1, 200], np.int32)}, dict(ref, counts=np.array([2, 1, 200], np.int32)), "invisible", vis=np.array([1, 0, 1]))
