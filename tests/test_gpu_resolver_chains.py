"""The greedy match resolvers (resolve_super and its callers, k_track.hip) on deep dependency chains: the domino scenes of case_tables.py, whose
conditions test_case_tables.py holds with the oracle alone -- one chain of 95 queries through find_matches (fixpoint depth 96), five chains of 19 at
once through row_match (depth 20), a chain cut in two by a super-chunk that ends on the list area, its second half lying across local query 1 024
(depths 48 and 49), and the chain through update_staged's scan (depth 96).  Every frame is compared in full (diff_frame: features, row pairs,
matches, map, staged set and counts, bit for bit) and in its pose; the device's own iteration count (debug_stamps()[26], k_early_mid's deepest
super-chunk) proves that the map chains ran as deep as the recipe says."""
import gc
import threading

import pytest

from case_tables import DOMINO_MIN_DEPTH, STAGED_CHAIN_DROPPED, domino_scene
from parity_util import POSE_TOL, diff_frame, make_case, pose_errors

pytestmark = pytest.mark.gpu

ST_ITER_SUM, ST_CHUNKS, ST_SLOW, ST_ITER_MAX, ST_QUERIES = 18, 24, 25, 26, 27      # debug_stamps(): k_early_mid's resolver (k_track.hip, resolve_body)


def _deepest(st, binned):
    """the deepest super-chunk of k_early_mid's resolver.  With LVT_AMD_BINNED_LISTS=1 the row-list kernel of the early stream keeps its own cycle
    stamps in dbg[26..31] (k_lists.hip) and may have overwritten the resolver's [26] and [27] by the time the frame is read: there the iteration sum
    over the super-chunks divided by their number stands in, a lower bound of the deepest one ([18] and [24] are the resolver's alone)"""
    if binned == "0":
        return int(st[ST_ITER_MAX])
    return -(-int(st[ST_ITER_SUM]) // int(st[ST_CHUNKS]))


def _run(hip_lib, name):
    """the scene through a HIP handle and an oracle side by side; per frame (oracle counts, debug stamps)"""
    from oracle import pyoracle as O
    prm, frames, info = domino_scene(name)
    hip, orc = hip_lib.LvtSystem.create(prm, 1), O.Oracle(prm, 1)
    rows = []
    for i, f in enumerate(frames):
        Ro, to = orc.track_with_external_corners(*f)
        Rh, th = hip.track_with_external_corners(*f)
        msgs = diff_frame(hip, orc)
        assert not msgs, f"{name} frame {i}: {msgs[:6]}"
        e_t, e_R = pose_errors(Rh, th, Ro, to)
        assert e_t <= POSE_TOL and e_R <= POSE_TOL, f"{name} frame {i}: pose e_t={e_t:.3e} e_R={e_R:.3e}"
        assert hip.get_state() == orc.status == 2 and hip.last_error() == ""
        rows.append((orc.counts(), hip.debug_stamps().copy()))
    hip.close()
    return info, rows


@pytest.mark.parametrize("binned", ["0", "1"], ids=["wave_per_query_lists", "binned_list_kernel"])
def test_map_chain(hip_lib, oracle_lib, monkeypatch, binned):
    """`map_chain`: frame 0 is `row_chain` (k_triangulate's resolver: five chains of 19, all 100 corners paired and triangulated), frame 1 resolves the
    chain of 95 in k_track_mid (the map is new: nothing for the early stream yet), frame 2 in k_early_mid, whose stamps say how deep it went"""
    monkeypatch.setenv("LVT_AMD_BINNED_LISTS", binned)
    info, rows = _run(hip_lib, "map_chain")
    assert rows[0][0]["n_row_matches"] == rows[0][0]["n_triangulated"] == 100
    assert [co["n_matches"] for co, _ in rows] == [0, 100, 100]
    st = rows[2][1]
    print("map_chain stamps: chunks", int(st[ST_CHUNKS]), "queries", int(st[ST_QUERIES]), "deepest", int(st[ST_ITER_MAX]), "sum", int(st[ST_ITER_SUM]), "fixpoint cycles", int(st[19]))
    assert st[ST_CHUNKS] == 1 and st[ST_SLOW] == 0 and (binned == "1" or st[ST_QUERIES] == 100)
    assert _deepest(st, binned) >= DOMINO_MIN_DEPTH["map_chain"] == 64, _deepest(st, binned)


@pytest.mark.parametrize("binned", ["0", "1"], ids=["wave_per_query_lists", "binned_list_kernel"])
def test_chain_across_super_chunks(hip_lib, oracle_lib, monkeypatch, binned):
    """`chain_across_super_chunks`: 1 663 map points in two super-chunks, the first ended by the list area; the second half of the chain starts from a
    permanent mark and runs from the threads' first queries into their second ones"""
    monkeypatch.setenv("LVT_AMD_BINNED_LISTS", binned)
    info, rows = _run(hip_lib, "chain_across_super_chunks")
    assert [co["n_matches"] for co, _ in rows] == [0, 1663, 1663] and rows[0][0]["map_size"] == info["n_corners"] == 1663
    st = rows[2][1]
    print("chain_across_super_chunks stamps: chunks", int(st[ST_CHUNKS]), "queries", int(st[ST_QUERIES]), "deepest", int(st[ST_ITER_MAX]), "sum", int(st[ST_ITER_SUM]),
          "fixpoint cycles", int(st[19]))
    assert st[ST_CHUNKS] >= 2 and st[ST_SLOW] == 0 and (binned == "1" or st[ST_QUERIES] == 1663)
    assert _deepest(st, binned) >= DOMINO_MIN_DEPTH["chain_across_super_chunks"] == 32, _deepest(st, binned)
    assert st[ST_ITER_SUM] >= 2 * DOMINO_MIN_DEPTH["chain_across_super_chunks"], int(st[ST_ITER_SUM])      # both halves ran deep, not one of them


def test_staged_chain(hip_lib, oracle_lib):
    """`staged_chain`: the chain of 95 through update_staged's resolver at frame 2 (staged_body exports no iteration count: the depth is the recipe's
    condition, the result is held here): 97 promotions in chain order behind the 1 563 map points, three staged points erased"""
    info, rows = _run(hip_lib, "staged_chain")
    co = rows[2][0]
    assert rows[1][0]["staged_size"] == 100 and (co["n_staged_promoted"], co["n_staged_erased"], co["map_size"]) == (97, STAGED_CHAIN_DROPPED, 1660)


def test_map_chain_on_a_seat_of_the_lockstep_pool(hip_lib, oracle_lib):
    """two pooled handles, seats of one lock-step launch chain (k_hamming_batched_lists builds the lists, the same resolvers decide): seat 0 runs the
    `map_chain` scene through the external-corner entry (a batch has none, and the detector does not return the nodes in chain order), seat 1 an
    ordinary KITTI-shaped world of the same size under the same parameters.  Each seat against its own oracle: every frame's full diff and pose."""
    from oracle import pyoracle as O
    prm, frames, info = domino_scene("map_chain")
    world, prm1, _ = make_case("kitti", 17, 1.0)
    assert (world.W, world.H) == (prm.img_width, prm.img_height) and (prm1.fx, prm1.fy, prm1.cx, prm1.cy, prm1.baseline) == (prm.fx, prm.fy, prm.cx, prm.cy, prm.baseline)
    frames = list(frames) + [frames[-1]]
    plain = [world.render_stereo(i) for i in range(len(frames))]
    gc.collect()        # (seats share their pool's parameters: a forgotten seat of an earlier test must be gone before these two found a pool of their own)
    hs = [hip_lib.LvtSystem.create(prm, 1, pooled=True) for _ in range(2)]
    assert all(h.ordering() == "pooled" for h in hs)
    orcs = [O.Oracle(prm, 1) for _ in range(2)]
    fails, n_matches = [[], []], [[], []]

    def work(k):
        for i in range(len(frames)):
            if k == 0:
                Ro, to = orcs[k].track_with_external_corners(*frames[i])
                Rh, th = hs[k].track_with_external_corners(*frames[i])
            else:
                Ro, to = orcs[k].track(*plain[i])
                Rh, th = hs[k].track(*plain[i])
            msgs = diff_frame(hs[k], orcs[k])
            e_t, e_R = pose_errors(Rh, th, Ro, to)
            if e_t > POSE_TOL or e_R > POSE_TOL:
                msgs.append(f"pose e_t={e_t:.3e} e_R={e_R:.3e}")
            if hs[k].get_state() != 2 or orcs[k].status != 2:
                msgs.append(f"status {hs[k].get_state()} / {orcs[k].status}")
            if msgs:
                fails[k].append((i, msgs[:4]))
                return
            n_matches[k].append(orcs[k].counts()["n_matches"])

    ths = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ths: t.start()
    for t in ths: t.join()
    for h in hs: h.close()
    assert fails == [[], []], fails
    assert n_matches[0] == [0, 100, 100, 100] and min(n_matches[1][1:]) > 300, n_matches
