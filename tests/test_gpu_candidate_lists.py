"""-m gpu: the candidate lists every match starts from, list by list.  Five pieces of code build them -- candidates_body<ROW> (k_candidates, and the fall-back
behind the binned kernel), candidates_body<MAP, PROJECT> (k_early_map / k_match_map, split at early_done), candidates_body<STAGED> (k_candidates behind k_pnp),
candidates_body<MAP> pass 2 (inside k_track_mid) and k_hamming_batched_lists<ROW / MAP> (k_lists.hip, the default of every lock-step batch) -- and the rest of
the suite sees them only through what the greedy resolvers make of them.  Here lvt_amd_get_candidate_lists reads them back and tests/lists_util.py restates
them: keys (distance << 16 | index) ascending, the full count, nothing for an invisible point.  The map / staged references take the device's own projections
as queries, so the list stage is exact given its input: everything is integers and equality is the claim.

Every case of tests/list_cases.py (tests/test_list_cases.py shows with the oracle alone that each plants what it claims) runs on a single-sequence handle under
LVT_AMD_BINNED_LISTS=0 and =1 (read at creation); both builders must give the reference's lists, and each other's arrays."""
import ctypes

import numpy as np
import pytest

import list_cases as LC
import lists_util as LU

pytestmark = pytest.mark.gpu


def _create(hip_lib, monkeypatch, case, binned):
    monkeypatch.setenv("LVT_AMD_ORDERING", "polling")          # the early stream lists the early map points and the rows: the path of the benchmark
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("LVT_AMD_BINNED_LISTS", "1" if binned else "0")
    sys_ = hip_lib.LvtSystem.create(case["prm"], 1)
    assert sys_.ordering() == "polling"
    return sys_


def _same_arrays(a, b, tag):
    """the two builders against each other: counts, and every specified key"""
    assert np.array_equal(a["counts"], b["counts"]), tag
    spec = np.arange(LU.KC)[None, :] < np.where(a["counts"] <= LU.KC, a["counts"], 0)[:, None]
    assert np.array_equal(a["keys"][spec], b["keys"][spec]), tag


@pytest.mark.parametrize("name", sorted(LC.ROW_CASES))
def test_row_lists(hip_lib, monkeypatch, name):
    case = LC.ROW_CASES[name]()
    got = {}
    for binned in (0, 1):
        sys_ = _create(hip_lib, monkeypatch, case, binned)
        sys_.track_with_external_corners(*case["frames"][0])
        assert sys_.last_error() == "", sys_.last_error()
        (xl, _, dl), (xr, _, dr) = sys_.features(0), sys_.features(1)
        g = sys_.candidate_lists("row")
        cnt = sys_.counts()
        sys_.close()
        ref = LU.row_lists(xl, dl, xr, dr, case["H"])
        LC.check_row_claims(case, xl, xr, ref)
        info = g["info"]
        print(name, "binned", binned, info, "lists", len(ref["counts"]), "longest", int(ref["counts"].max(initial=0)), "ties", LU.equal_distance_neighbours(ref["full"]))
        assert info["binned"] == binned and info["kc"] == LU.KC and info["n"] == len(xl) == cnt["n_left"]
        assert info["stood_down_row"] == (case["expect"]["stood_down_row"] if binned else 0), info
        assert cnt["row_fallback"] == case["expect"].get("row_fallback", 0), cnt
        assert len(g["proj"]) == 0 and len(g["vis"]) == 0
        LU.hold(g, ref, f"{name} ({case['plants']}) binned={binned}")
        got[binned] = g
    _same_arrays(got[0], got[1], name)


@pytest.mark.parametrize("name", sorted(LC.MAP_CASES))
def test_map_lists(hip_lib, monkeypatch, name):
    case = LC.MAP_CASES[name]()
    c, exp = case["claims"], case["expect"]
    staged = c.get("staged", False)
    got = {}
    for binned in (0, 1):
        sys_ = _create(hip_lib, monkeypatch, case, binned)
        for f in case["frames"][:2]:
            sys_.track_with_external_corners(*f)
        _, _, _, mdesc = sys_.map()
        _, _, sdesc = sys_.staged()
        sys_.track_with_external_corners(*case["frames"][2])
        assert sys_.get_state() == 2 and sys_.last_error() == "", sys_.last_error()       # a tracked, non-first frame
        xy, _, desc = sys_.features(0)
        cnt = sys_.counts()
        lists = {"map": sys_.candidate_lists("map"), "staged": sys_.candidate_lists("staged")}
        sys_.close()
        info = lists["map"]["info"]
        print(name, "binned", binned, info, cnt)
        assert info["binned"] == binned and info["n"] == cnt["map_size_at_match"] == len(mdesc)
        assert info["pass2"] == cnt["second_pass"] == exp["pass2"]
        assert info["stood_down_map"] == (exp["stood_down_map"] if binned else 0), info
        assert lists["staged"]["info"]["n"] == len(sdesc) == (c["n1"] if staged else 0)     # the staged count when the lists were built = after the previous frame
        for which, qd in (("map", mdesc),) + ((("staged", sdesc),) if staged else ()):
            g = lists[which]
            ref = LU.track_lists(g["proj"], g["vis"], qd, xy, desc, case["radius"], case["W"], case["H"], pass2=bool(exp["pass2"]) and which == "map")
            LC.check_map_claims(case, g["proj"], g["vis"], xy, ref, n_early=info["n_early"], which=which)
            held = LU.hold(g, ref, f"{name} {which} ({case['plants']}) binned={binned}", vis=g["vis"])
            print("  ", which, "lists", len(ref["counts"]), "longest", int(ref["counts"].max()), "keys held", held, "ties", LU.equal_distance_neighbours(ref["full"]))
            got[binned, which] = g
    for which in ("map",) + (("staged",) if staged else ()):
        _same_arrays(got[0, which], got[1, which], (name, which))
        assert np.array_equal(got[0, which]["proj"], got[1, which]["proj"]) and np.array_equal(got[0, which]["vis"], got[1, which]["vis"])


def test_lists_that_were_not_built_and_refusals(hip_lib, monkeypatch):
    """before the first frame and on it: no map or staged lists (n = 0), the row lists are there; -1 for no handle, memory that is no handle, a batch, a `which`
    out of range and a cap below n"""
    L = hip_lib.load_library()
    case = LC.ROW_CASES["row_band_edges"]()
    sys_ = _create(hip_lib, monkeypatch, case, 1)
    for which in ("map", "staged", "row"):
        assert sys_.candidate_lists(which)["info"]["n"] == 0
    sys_.track_with_external_corners(*case["frames"][0])
    assert [sys_.candidate_lists(w)["info"]["n"] for w in ("map", "staged", "row")] == [0, 0, len(sys_.features(0)[0])]
    n = len(sys_.features(0)[0])
    keys = np.zeros((n, LU.KC), np.uint32); counts = np.full(n, -7, np.int32); info = np.zeros(8, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    call = lambda h, w, cap: L.lvt_amd_get_candidate_lists(h, w, p(keys), p(counts), None, None, cap, p(info))  # noqa: E731
    not_a_handle = np.zeros(64, np.uint64)
    assert call(None, 2, n) == -1 and call(p(not_a_handle), 2, n) == -1
    assert call(sys_._h, 3, n) == -1 and call(sys_._h, -1, n) == -1
    assert call(sys_._h, 2, n - 1) == -1 and (counts == -7).all() and info[6] == n          # too small: nothing copied, the record says how many
    batch = hip_lib.LvtBatch(case["prm"], 2)
    assert call(batch._h, 2, n) == -1 and (counts == -7).all()
    batch.close()
    assert call(sys_._h, 2, n) == n and (counts >= 0).all()
    with pytest.raises(ValueError):
        sys_.candidate_lists(5)
    sys_.close()
