"""The per-frame map kernels from 10 000 map points to past their capacity (MAP_MAX = 32 768, lvt_dev.h), frame by frame against the oracle: the
recipes of case_tables.py ("the map kernels from 10k points to past capacity"; test_case_tables.py holds them to their sizes with the oracle alone).
Past the capacity the oracle runs with the same capacities (Oracle.set_capacities: the first 32 768 points in append order, the cut reported in the
frame's overflow count) -- include/lvt_c.h, "capacities".  Every frame of every test is compared in full (diff_frame) and in its pose."""
import pytest

import numpy as np

from case_tables import MAP_MAX, MAPCAP_RECIPES, RES_THREADS, STAGED_MAX, mapcap_case, mapcap_track, mapseam_case
from parity_util import POSE_TOL, diff_frame, make_case, pose_errors

pytestmark = pytest.mark.gpu

QCAP = 2048                  # k_track.hip: queries of one super-chunk; it ends earlier when its packed candidates fill LCAP
# what diff_frame says of a frame whose map was cut -- the report itself -- and nothing else
OVERFLOW_MSGS = ("hip error: capacity overflow mask 0x8 in sequence 0", "overflow mask 8")
ST_CHUNKS, ST_QUERIES = 24, 27       # debug_stamps(): k_early_mid's super-chunks and its queries (the points that have candidates among
                                     # [0, map size behind the previous frame's cull))


def _compare(hip, orc, frames, first=0):
    """the frames through both systems; per frame the full diff (only a reported cut may differ, and then the oracle must have cut as well) and the
    pose.  Returns per frame (oracle counts, hip counts, debug stamps)."""
    rows = []
    for i, f in enumerate(frames, first):
        Ro, to = mapcap_track(orc, f)
        Rh, th = mapcap_track(hip, f)
        msgs = diff_frame(hip, orc)
        co = orc.counts()
        if co["overflow"]:
            assert co["overflow"] == 8, (i, co)
            for m in OVERFLOW_MSGS:
                assert m in msgs, f"frame {i}: no '{m}' in {msgs[:6]}"
                msgs.remove(m)
        assert not msgs, f"frame {i}: {msgs[:6]}"
        e_t, e_R = pose_errors(Rh, th, Ro, to)
        assert e_t <= POSE_TOL and e_R <= POSE_TOL, f"frame {i}: pose e_t={e_t:.3e} e_R={e_R:.3e}"
        assert hip.get_state() == orc.status == 2, (i, hip.get_state(), orc.status)
        rows.append((co, hip.counts(), hip.debug_stamps().copy()))
    return rows


def _systems(hip_lib, name, capped, n_frames=None):
    from oracle import pyoracle as O
    prm, frames = mapcap_case(name, n_frames)
    orc = O.Oracle(prm, 1)
    if capped:
        orc.set_capacities(MAP_MAX, STAGED_MAX)
    return hip_lib.LvtSystem.create(prm, 1), orc, frames


def _lcap_cut(rows):
    """frames whose early resolver walked more super-chunks than its queries need at QCAP apiece: chunks ended on the candidate area (LCAP)"""
    return [i for i, (_, _, st) in enumerate(rows) if st[ST_CHUNKS] > -(-int(st[ST_QUERIES]) // QCAP)]


def test_steady_state_of_28000_points_culling_3000_a_frame(hip_lib, oracle_lib):
    """`steady`, the unmodified oracle: from frame 8 on bookkeep_cull_large runs on 26 700 to 28 100 points and culls 3 250 to 3 600 of them per frame,
    its compaction moving ~24 500 survivors; the resolvers walk the map in super-chunks that end on LCAP (~17 candidates per point).  The early
    resolver's own share is the map behind the previous frame's cull: 23 500 to 24 900 queries here (at more than 25 000: test_triangulation_past_the_capacity)"""
    hip, orc, frames = _systems(hip_lib, "steady", capped=False)
    rows = _compare(hip, orc, frames)
    assert len(rows) == 14
    for i in range(8, 14):
        (co, ch, st), prev = rows[i], rows[i - 1][1]
        assert ch["map_size_at_match"] > 25000 and ch["n_culled"] > 3000 and ch["overflow"] == 0, ch
        # its queries: the map behind the previous frame's cull, but for the points without a candidate.  A 51 x 51 px window holds ~17 of the frame's
        # 3 700 fresh corners (half of that at the edge of their area), ~12 of the 300 fixed ones in their strip: a point in thousands has none
        early = prev["map_size_at_match"] - prev["n_culled"]
        assert early > 23000 and 0.95 * early < st[ST_QUERIES] <= early, (i, early, st[ST_QUERIES])
    assert max(ch["map_size"] for _, ch, _ in rows) <= MAP_MAX
    assert _lcap_cut(rows), [(int(st[ST_CHUNKS]), int(st[ST_QUERIES])) for _, _, st in rows]


def test_triangulation_past_the_capacity(hip_lib, oracle_lib):
    """`direct` against the oracle with the same capacities: k_triangulate appends past MAP_MAX at frame 9 -- the first 32 768 points in append order are
    the map, the cut is reported -- and the frames behind it run every map kernel at exactly MAP_MAX points: all 32 chunks of bookkeep_cull_large,
    n_keep = 32 768 in the high half of its packed scan, an early resolver with more than 25 000 queries.  Then reset() and a clean start."""
    hip, orc, frames = _systems(hip_lib, "direct", capped=True)
    rows = _compare(hip, orc, frames)
    assert len(rows) == 12
    assert all(ch["overflow"] == 0 and ch["map_size"] < MAP_MAX for _, ch, _ in rows[:9])
    for co, ch, st in rows[9:]:
        assert ch["overflow"] == 8 and ch["map_size"] == co["map_size"] == MAP_MAX, ch
    for co, ch, st in rows[10:]:
        assert ch["map_size_at_match"] == MAP_MAX and ch["n_culled"] == 0
        assert st[ST_QUERIES] > 25000, st[ST_QUERIES]
    assert max(st[ST_QUERIES] for _, _, st in rows) > 25000 and _lcap_cut(rows)
    hip.reset(); orc.reset()
    _, again = mapcap_case("direct", 3)
    rows = _compare(hip, orc, again)
    assert all(ch["overflow"] == 0 for _, ch, _ in rows) and hip.last_error() == ""
    assert [ch["map_size"] for _, ch, _ in rows] == [co["map_size"] for co, _, _ in rows] and rows[2][1]["map_size"] > 10000


def test_overflow_followed_by_recovery(hip_lib, oracle_lib):
    """`direct` with untracked_threshold 10: the map is cut at frames 9 and 10, the cull of frame 10 onwards takes more than 3 000 points per frame out
    of a full map, and from frame 11 on nothing overflows and nothing is reported"""
    hip, orc, frames = _systems(hip_lib, "direct_recover", capped=True)
    rows = _compare(hip, orc, frames)
    ovf = [i for i, (_, ch, _) in enumerate(rows) if ch["overflow"]]
    assert ovf and len(rows) == 14
    later = [i for i, (_, ch, _) in enumerate(rows) if i > ovf[0] and ch["overflow"] == 0 and ch["n_culled"] > 3000]
    assert later, [(ch["overflow"], ch["n_culled"]) for _, ch, _ in rows]
    assert any(ch["map_size_at_match"] == MAP_MAX and ch["n_culled"] > 3000 for _, ch, _ in rows)       # a cull out of all 32 chunks
    assert hip.last_error() == "" and rows[-1][1]["overflow"] == 0


def test_promotion_past_the_capacity(hip_lib, oracle_lib):
    """`promotion` against the capped oracle: staged sets of 3 000 to 3 600 points, promoted at once on every odd frame (staged_body over several
    super-chunks, its second scan pair, matched_before / promoted_before carried across them); at frame 19 the promotions pass MAP_MAX: the first
    1 662 fit, the others are dropped and leave the staged set all the same"""
    hip, orc, frames = _systems(hip_lib, "promotion", capped=True)
    staged_18 = None
    rows = []
    for i, f in enumerate(frames):
        rows += _compare(hip, orc, [f], first=i)
        if i == 18:
            staged_18 = hip.staged()[0]
        if i == 19:
            co, ch, _ = rows[-1]
            assert ch["overflow"] == 8 and ch["map_size"] == MAP_MAX
            assert ch["n_staged_promoted"] == co["n_staged_promoted"] > rows[18][1]["staged_size"] - 100 > 2048
            fits = MAP_MAX - rows[18][1]["map_size"]
            assert 0 < fits < ch["n_staged_promoted"]                     # some of this frame's promotions fit, the others were dropped
            was = {p.tobytes() for p in staged_18}
            assert len(was) == len(staged_18) == rows[18][1]["staged_size"]
            assert not [p for p in hip.staged()[0] if p.tobytes() in was], "a staged point outlived its promotion"
            # of the points staged at frame 18 exactly those that fit are in the map, behind everything else
            xyz = hip.map()[0]
            assert [j for j, p in enumerate(xyz) if p.tobytes() in was] == list(range(MAP_MAX - fits, MAP_MAX))
    assert len(rows) == 22
    assert [i for i, (_, ch, _) in enumerate(rows) if ch["overflow"]] == [19, 20, 21]
    assert sum(1 for _, ch, _ in rows if ch["staged_size"] > 2048) >= 5 and sum(1 for _, ch, _ in rows if ch["n_staged_promoted"] > 2048) >= 5


def test_capacity_cut_in_one_sequence_of_a_lockstep_batch(hip_lib, oracle_lib):
    """`detector` as sequence 0 of a lock-step batch of two (the map kernels' instance that reads its sequence from the device array), frames in HBM;
    sequence 1 is an ordinary KITTI-shaped world.  Each sequence against its own oracle, sequence 0's capped: counts, status and pose of every frame.
    Sequence 0's map is cut from frame 16 on; sequence 1 never shows an overflow bit or a differing count"""
    import torch
    from oracle import pyoracle as O
    n = MAPCAP_RECIPES["detector"][3]
    prm, frames0 = mapcap_case("detector")
    world, prm1, _ = make_case("kitti", 17, 1.0)
    W, H = world.W, world.H
    assert (W, H) == (prm.img_width, prm.img_height) and (prm1.fx, prm1.fy, prm1.cx, prm1.cy, prm1.baseline) == (prm.fx, prm.fy, prm.cx, prm.cy, prm.baseline)
    pitch = ((W + 63) // 64) * 64
    dev = torch.zeros((2, 2, H, pitch), dtype=torch.uint8, device="cuda")
    batch = hip_lib.LvtBatch(prm, 2)
    orcs = [O.Oracle(prm, 1), O.Oracle(prm, 1)]
    orcs[0].set_capacities(MAP_MAX, STAGED_MAX)
    seen = []
    for i, f in enumerate(frames0):
        pair = [(f[0], f[1]), world.render_stereo(i)]
        for s in range(2):
            for e in range(2):
                dev[s, e, :, :W] = torch.from_numpy(pair[s][e]).cuda()
        torch.cuda.synchronize()
        batch.track_device_async([dev[s, 0].data_ptr() for s in range(2)], [dev[s, 1].data_ptr() for s in range(2)], H, W, pitch)
        Rb, tb, st = batch.wait()
        for s in range(2):
            Ro, to = orcs[s].track(*pair[s])
            e_t, e_R = pose_errors(Rb[s], tb[s], Ro, to)
            assert e_t <= POSE_TOL and e_R <= POSE_TOL and st[s] == orcs[s].status == 2, f"sequence {s} frame {i}: {e_t:.2e} {e_R:.2e}"
            co, ch = orcs[s].counts(), batch.counts(s)
            bad = {k: (ch.get(k), v) for k, v in co.items() if ch.get(k) != v}
            assert not bad, f"sequence {s} frame {i}: counters (hip, oracle) {bad}"
        c0, c1 = batch.counts(0), batch.counts(1)
        assert c1["overflow"] == 0 and c1["map_size"] < MAP_MAX // 2
        assert batch.last_error() == ("capacity overflow mask 0x8 in sequence 0" if c0["overflow"] else ""), (i, batch.last_error())
        seen.append(c0["overflow"])
    assert len(seen) == n == 18 and seen == [0] * 16 + [8, 8] and batch.counts(0)["map_size"] == MAP_MAX


def test_bookkeeping_either_side_of_1024_points(hip_lib, oracle_lib):
    """`seam` (case_tables.py; test_case_tables.py holds its sizes): k_track_mid's two bookkeeping bodies in turn -- bookkeep_cull_small on a map of 938
    points, bookkeep_cull_large on 1 043 (two chunks, the second nearly empty, a cull of 591), the small one again on what that left, the large one on
    1 115 and 1 102 -- every frame compared in full and in its pose"""
    from oracle import pyoracle as O
    prm, frames = mapseam_case("seam")
    hip = hip_lib.LvtSystem.create(prm, 1)
    rows = _compare(hip, O.Oracle(prm, 1), frames)
    hip.close()
    at_match = [ch["map_size_at_match"] for _, ch, _ in rows]
    assert any(896 < m <= RES_THREADS for m in at_match) and any(RES_THREADS < m <= 1152 for m in at_match), at_match
    assert [m > RES_THREADS for m in at_match[1:]] == [False, True, False, False, True, True], at_match
    assert all(ch["n_culled"] > 90 for _, ch, _ in rows[2:])


def test_lost_on_a_map_of_more_than_1024_points(hip_lib, oracle_lib):
    """`lost`: LOST decided by bookkeep_cull_large (1 420 points at match time), whose LOST branch applies the bookkeeping in place, compacts nothing and
    returns ahead of its last barrier: the frame's full diff -- counters and ages of the map are those in-place writes --, then the state 3 latch: the
    last pose again, the map untouched"""
    from oracle import pyoracle as O
    prm, frames = mapseam_case("lost")
    hip, orc = hip_lib.LvtSystem.create(prm, 1), O.Oracle(prm, 1)
    _compare(hip, orc, frames[:3])
    before = hip.map()
    Ro, to = mapcap_track(orc, frames[3])
    Rh, th = mapcap_track(hip, frames[3])
    msgs = diff_frame(hip, orc)
    assert not msgs, msgs[:6]
    ch = hip.counts()
    assert hip.get_state() == orc.status == 3 and ch["map_size_at_match"] > RES_THREADS and ch["second_pass"] == 1 and ch["n_matches"] < prm.min_num_matches_for_tracking
    after, want = hip.map(), orc.map()
    assert all(np.array_equal(a, b) for a, b in zip(after[1:], want[1:])) and len(after[0]) == len(before[0]) == ch["map_size_at_match"]
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[3], before[3])              # nothing moved ...
    assert int((after[1] != before[1]).sum()) > 100 and int((after[2] - before[2]).sum()) == ch["n_matches"]      # ... counters and ages stepped
    last = th.copy()
    Ro, to = mapcap_track(orc, frames[4]); Rh, th = mapcap_track(hip, frames[4])                     # LOST is sticky: the last pose, nothing is computed
    assert hip.get_state() == orc.status == 3 and np.array_equal(th, last) and np.allclose(th, to, atol=1e-9)
    still, error = hip.map(), hip.last_error()
    hip.close()
    assert all(np.array_equal(a, b) for a, b in zip(still, after)) and error == ""
