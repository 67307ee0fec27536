"""CPU tier: the case tables of the k_pnp / k_triangulate edge tests (case_tables.py) cannot rot.  With the oracle alone: the inputs still take the
branches the GPU tests rely on -- so a GPU test that passes has compared what its docstring says it compares."""
import numpy as np
import pytest

import lvt_amd
from case_tables import (MAP_MAX, MAPCAP_RECIPES, STAGED_MAX, mapcap_case, mapcap_track)
from case_tables import (RGBD16_SETS, RGBD_BARREL, RGBD_BARREL_FRAMES, RGBD_FAR, RGBD_NEAR, RGBD_NODEPTH, RGBD_PLANT_FRAMES, RGBD_RETRY, RGBD_RETRY_FRAMES,
                         rgbd_backproject, rgbd_depth_classes, rgbd_nodepth_script, rgbd_outside, rgbd_planted, rgbd_world)
from case_tables import (DENSE_MIN_UNSTAGED_FRAMES, KITTI_DENSE_UNSTAGED, PNP_EDGE_COUNTS, PNP_HARD, PNP_HARD_UNSTAGED, PNP_INTRINSICS, PNP_STAGE_MAX,
                         STAIRCASE, pnp_edge_case, pnp_hard_case, pnp_prior_cases, staircase, staircase_band_counts, staircase_expected, trace_noise)


def test_edge_count_cases_take_no_borderline_decision(oracle_lib):
    """29 edge counts x 3 intrinsics: no gate decision of the oracle within 1e-8 of the threshold (the nearest stays 1.4e-2 away), 10 solve calls
    for every n >= 3, and the noise-level endings of n = 1, 2 where the GPU test expects them"""
    assert len(PNP_EDGE_COUNTS) * len(PNP_INTRINSICS) == 87
    assert {0, 1, 2, 64, 256, 768, PNP_STAGE_MAX, PNP_STAGE_MAX + 1, 4096} <= set(PNP_EDGE_COUNTS)
    for name in PNP_INTRINSICS:
        for n in PNP_EDGE_COUNTS:
            prm, X, uv, q0, p0 = pnp_edge_case(name, n)
            q, p, marks, tr = oracle_lib.pnp(prm, q0, p0, X, uv)
            o = oracle_lib.pnp
            assert o.last_borderline == 0, (name, n)
            if n == 0:
                assert o.last_solve_calls == 0 and len(tr) == 0 and np.array_equal(q, [1, 0, 0, 0]) and np.array_equal(p, [0, 0, 0])
                continue
            assert o.last_min_margin >= 1.4e-2, (name, n, o.last_min_margin)
            if n >= 3:
                assert o.last_solve_calls == 10 and o.last_terminates == 0, (name, n, o.last_solve_calls)
                assert trace_noise(tr) >= 3, (name, n)
            if n >= 9:
                assert 0 < marks.sum() < n, (name, n)           # the gates demote the planted outliers and keep the rest
    prm = lvt_amd.tum_params()
    assert prm.fx != prm.fy
    # n = 1: 5 trials, 2 rejected, both passes Terminate, the first noise-level trial is the fourth
    prm, X, uv, q0, p0 = pnp_edge_case("kitti", 1)
    _, _, _, tr = oracle_lib.pnp(prm, q0, p0, X, uv)
    assert (oracle_lib.pnp.last_trials, oracle_lib.pnp.last_rejections, oracle_lib.pnp.last_terminates, trace_noise(tr)) == (5, 2, 2, 3)


def test_prior_cases_are_one_solve(oracle_lib):
    """q, -q, 3 q and the unnormalised quaternion with w < 0: one pose, the same marks and counters on the oracle; a tenth of the points behind the camera"""
    prm = lvt_amd.kitti_params()
    labels = []
    for label, X, uv, priors, p0 in pnp_prior_cases(prm):
        labels.append((label, len(X)))
        ref = None
        for q0 in priors:
            q, p, marks, tr = oracle_lib.pnp(prm, q0, p0, X, uv)
            o = oracle_lib.pnp
            got = (o.last_solve_calls, o.last_trials, o.last_rejections, o.last_terminates, o.last_borderline)
            assert o.last_borderline == 0 and o.last_min_margin > 1e-2
            if ref is None:
                ref = (q, p, marks, got)
            assert np.abs(q - ref[0]).max() < 1e-13 and np.abs(p - ref[1]).max() < 1e-13 and np.array_equal(marks, ref[2]) and got == ref[3], label
        if label.startswith("behind"):
            assert len(priors) == 4 and priors[3][0] < 0 and abs(np.linalg.norm(priors[2]) - 3) < 1e-12 and (X[:, 2] < 0).sum() >= len(X) // 20
        else:
            e2 = (oracle_lib.pnp.last_err ** 2).sum(axis=1)     # outliers over five decades
            assert e2.max() > 1e10 and sum(((e2 > 10.0 ** (2 * k)) & (e2 < 10.0 ** (2 * k + 2))).any() for k in range(1, 5)) == 4
    assert labels == [("behind_40", 40), ("behind_300", 300), ("behind_1700", 1700), ("graded_outliers", 600)]


def _tally(oracle_lib, table):
    prm = lvt_amd.kitti_params()
    rows = []
    for case in table:
        X, uv, q0, p0 = pnp_hard_case(prm, *case)
        _, _, _, tr = oracle_lib.pnp(prm, q0, p0, X, uv)
        o = oracle_lib.pnp
        rows.append(dict(case=case, full=trace_noise(tr) == len(tr), rej=o.last_rejections, term=o.last_terminates, nan=bool(np.isnan(tr).any()),
                         border=o.last_borderline))
    return rows


def test_hard_rows_take_their_branches(oracle_lib):
    rows = _tally(oracle_lib, PNP_HARD_UNSTAGED)
    assert all(r["case"][1] > PNP_STAGE_MAX and r["border"] == 0 for r in rows)
    assert {r["case"][1] for r in rows} == {1600, 2500, 4096}
    # the closing condition of test_pnp_hard_branches_above_the_staging_limit
    assert sum(r["full"] for r in rows) >= 3 and sum(r["rej"] for r in rows) > 0 and sum(r["nan"] for r in rows) > 0 and sum(r["term"] for r in rows) > 0
    # row by row what the table says of them: the first nine are comparable to their last trial and reject 1, 1, 3, 1, 1, 7, 3, 2, 2 trials, two of them
    # with a NaN step; the last four Terminate behind a noise-level trial
    assert [r["full"] for r in rows] == [True] * 9 + [False] * 4
    assert [r["rej"] for r in rows[:9]] == [1, 1, 3, 1, 1, 7, 3, 2, 2] and [r["nan"] for r in rows[:9]] == [False, False, False, True, False, True, False, False, False]
    assert [r["term"] for r in rows] == [0] * 9 + [1] * 4 and rows[12]["rej"] == 4
    # ... and the table below the staging limit still meets its test's closing condition
    old = _tally(oracle_lib, PNP_HARD)
    full = [r for r in old if r["full"]]
    assert sum(r["rej"] for r in old) > 0 and sum(r["term"] for r in old) > 0 and sum(r["nan"] for r in old) > 0 and len(full) >= 3
    assert sum(r["rej"] for r in full) > 0 and sum(r["term"] + r["nan"] for r in full) > 0


def test_dense_sequence_stays_above_the_staging_limit(oracle_lib):
    from parity_util import make_case
    name, kind, seed, scale, overrides, frames = KITTI_DENSE_UNSTAGED
    world, prm, sensor = make_case(kind, seed, scale, overrides)
    orc = oracle_lib.Oracle(prm, sensor)
    n_matches = []
    for i in frames:
        orc.track(*world.render_stereo(i))
        c = orc.counts()
        n_matches.append(c["n_matches"])
        assert orc.status == 2 and c["n_left"] <= 4096 and c["n_right"] <= 4096 and c["overflow"] == 0, (i, orc.status, c)
    assert n_matches == [0, 1386, 1572, 1667, 1745, 1754, 1750, 1800, 1786, 1810], n_matches
    assert sum(1 for m in n_matches if m > PNP_STAGE_MAX) >= DENSE_MIN_UNSTAGED_FRAMES
    # the same world under the defaults, its neighbour in the mixed batch, stays staged
    _, prm_default, _ = make_case(kind, seed, scale)
    orc = oracle_lib.Oracle(prm_default, sensor)
    for i in frames[:3]:
        orc.track(*world.render_stereo(i))
    assert 0 < orc.counts()["n_matches"] <= PNP_STAGE_MAX and orc.status == 2


@pytest.mark.parametrize("variant", list(STAIRCASE))
def test_staircase_bands(oracle_lib, variant):
    prm, L, R, cl, cr, bands = staircase(variant)
    orc = oracle_lib.Oracle(prm, 1)
    orc.track_with_external_corners(L, R, cl, cr)
    c = orc.counts()
    want = staircase_expected(prm, bands)
    assert c["n_left"] == c["n_right"] == len(cl) == 114 * len(bands)
    assert c["n_row_matches"] == sum(w[0] for w in want) and c["n_triangulated"] == c["map_size"] == sum(w[1] for w in want), c
    assert staircase_band_counts(prm, orc.map()[0], len(bands)) == [w[1] for w in want]
    if variant == "13_bands":
        assert (L.shape, c["n_row_matches"], c["map_size"]) == ((1222, 1241), 1482, 570)
        assert [d for (d, _), w in zip(bands, want) if w[1]] == [9.7, 12, 40, 150, 192.9]
    if variant == "11_bands":
        assert L.shape[0] + 1 <= 1100 < 1222 + 1          # LS_BINS (k_lists.hip): this one's row lists fit the binned kernel
    if variant == "row_band_edge":
        assert [w[0] for w in want] == [114, 114, 0, 114]


# ---- the map-capacity recipes (test_gpu_map_capacity.py) -------------------------------------------------------------------------------------------
def _mapcap_rows(oracle_lib, name, n_frames=None, capped=False):
    """the recipe through the oracle alone: TRACKING on every frame; one row of counters per frame"""
    prm, frames = mapcap_case(name, n_frames)
    orc = oracle_lib.Oracle(prm, 1)
    if capped:
        orc.set_capacities(MAP_MAX, STAGED_MAX)
    rows = []
    for i, f in enumerate(frames):
        mapcap_track(orc, f)
        assert orc.status == 2, (name, i, orc.status)
        rows.append(orc.counts())
        assert rows[-1]["staged_size"] <= max(rows[-1]["n_left"], 1), (name, i)      # a staged point owns a feature or goes: far below STAGED_MAX
    return rows, orc


def _first_past_capacity(rows):
    return next(i for i, c in enumerate(rows) if c["map_size"] > MAP_MAX)


def test_mapcap_steady_culls_thousands_above_25000_points(oracle_lib):
    rows, _ = _mapcap_rows(oracle_lib, "steady")
    assert len(rows) == MAPCAP_RECIPES["steady"][3] == 14
    assert [c["map_size"] for c in rows[:8]] == [3985, 7607, 11173, 14679, 18134, 21537, 24861, 28104]
    assert all(c["n_culled"] > 3000 and c["map_size_at_match"] > 25000 and c["map_size"] > 25000 for c in rows[-6:]), [(c["n_culled"], c["map_size"]) for c in rows]
    assert max(c["map_size"] for c in rows) <= MAP_MAX and all(c["overflow"] == 0 for c in rows)
    assert all(c["n_left"] <= 4096 and c["n_right"] <= 4096 for c in rows)


def test_mapcap_direct_passes_the_capacity_at_frame_9(oracle_lib):
    rows, orc = _mapcap_rows(oracle_lib, "direct", 11)
    assert _first_past_capacity(rows) == 9 and [rows[i]["map_size"] for i in (8, 9, 10)] == [31333, 34508, 37652]
    assert all(c["overflow"] == 0 and c["n_culled"] == 0 for c in rows)                  # the default: the reference's unbounded growth
    # the capacity option is the documented cut and nothing else: the same frames, the first MAP_MAX points of the unbounded map in append order
    capped, orc_c = _mapcap_rows(oracle_lib, "direct", 10, capped=True)
    assert capped[:9] == rows[:9]
    assert {k: v for k, v in capped[9].items() if k not in ("map_size", "overflow")} == {k: v for k, v in rows[9].items() if k not in ("map_size", "overflow")}
    assert capped[9]["map_size"] == MAP_MAX and capped[9]["overflow"] == 8
    prm, frames = mapcap_case("direct", 10)
    ref = oracle_lib.Oracle(prm, 1)
    for f in frames:
        mapcap_track(ref, f)
    for a, b in zip(orc_c.map(), ref.map()):
        assert len(a) == MAP_MAX < len(b) == 34508 and np.array_equal(a, b[:MAP_MAX])


def test_mapcap_direct_recovers_from_an_overflow(oracle_lib):
    """untracked_threshold 10: the first culls at frame 10; the capped oracle overflows, then culls its way back below the capacity"""
    rows, _ = _mapcap_rows(oracle_lib, "direct_recover", capped=True)
    assert [i for i, c in enumerate(rows) if c["n_culled"]][0] == 10
    ovf = [i for i, c in enumerate(rows) if c["overflow"]]
    assert ovf == [9, 10] and all(rows[i]["overflow"] == 8 and rows[i]["map_size"] == MAP_MAX for i in ovf)
    assert any(c["overflow"] == 0 and c["n_culled"] > 3000 for c in rows[ovf[0] + 1:])
    assert all(c["overflow"] == 0 and c["n_culled"] > 3000 and c["map_size"] < MAP_MAX for c in rows[11:]) and len(rows) == 14


def test_mapcap_promotion_passes_the_capacity_by_promotion_at_frame_19(oracle_lib):
    rows, _ = _mapcap_rows(oracle_lib, "promotion", 24)
    assert _first_past_capacity(rows) == 19 and (rows[18]["map_size"], rows[19]["map_size"], rows[19]["n_staged_promoted"]) == (31106, 34263, 3157)
    assert rows[19]["n_triangulated"] < 100 and rows[19]["staged_size"] < 100          # ... by promotion: what frame 19 triangulates is staged
    big = [i for i, c in enumerate(rows) if c["staged_size"] > 2048]
    assert len(big) >= 5 and big[:3] == [2, 4, 6], big
    assert sum(1 for c in rows if c["n_staged_promoted"] > 2048) >= 5                    # staged_body's second scan pair: more than RES_THREADS matched
    capped, orc = _mapcap_rows(oracle_lib, "promotion", capped=True)
    assert len(capped) == 22 and [i for i, c in enumerate(capped) if c["overflow"]] == [19, 20, 21]
    assert capped[19]["n_staged_promoted"] == 3157 and capped[19]["map_size"] == MAP_MAX and capped[19]["staged_size"] == rows[19]["staged_size"]


def test_mapcap_detector_passes_the_capacity_at_frame_16(oracle_lib):
    rows, _ = _mapcap_rows(oracle_lib, "detector", 17)
    assert _first_past_capacity(rows) == 16 and (rows[15]["map_size"], rows[16]["map_size"]) == (32280, 33829)
    assert all(3000 < c["n_left"] <= 4096 and 3000 < c["n_right"] <= 4096 for c in rows)
    assert all(1400 <= c["n_triangulated"] <= 2400 for c in rows[1:])


def test_oracle_capacity_option_cuts_all_three_append_sites(oracle_lib):
    """Oracle.set_capacities at small capacities, so that each append site cuts within six frames of `promotion`: triangulation into the map (frame 0),
    into the staged set (bit 16, frame 2), promotion (frames 2 and 3); the mask is the frame's own, and (0, 0) is the unbounded default again"""
    prm, frames = mapcap_case("promotion", 6)
    orc, ref = oracle_lib.Oracle(prm, 1), oracle_lib.Oracle(prm, 1)
    orc.set_capacities(3000, 2000)
    ref.set_capacities(3000, 2000); ref.set_capacities(0, 0)
    rows = []
    for f in frames:
        mapcap_track(orc, f); mapcap_track(ref, f)
        rows.append(orc.counts())
        assert ref.counts()["overflow"] == 0
    # (frame 1 stages the ~1 000 corners whose map points frame 0 cut; those of the fixed strip are matched and promoted at frame 2: bit 8 there too)
    assert [c["overflow"] for c in rows[:4]] == [8, 0, 24, 8] and rows[2]["n_staged_promoted"] > 0, [c["overflow"] for c in rows]
    assert rows[0]["n_triangulated"] == 3985 and rows[0]["map_size"] == 3000
    got, first = orc.map(), ref.map()
    assert all(np.array_equal(got[k][:3000], first[k][:3000]) for k in (0, 3))               # positions, descriptors: the first points in append order
    assert rows[2]["n_triangulated"] > 2000 == rows[2]["staged_size"] and rows[2]["map_size"] == 3000
    # frame 3: every matched staged point is promoted and none fits -- dropped, and gone from the staged set all the same
    # (what is staged behind it is what frame 3 triangulates: the corners whose points frame 2's staged cut had dropped)
    assert rows[3]["n_staged_promoted"] + rows[3]["n_staged_erased"] == 2000 and rows[3]["n_staged_promoted"] > 1900 and rows[3]["map_size"] == 3000
    assert rows[3]["staged_size"] == rows[3]["n_triangulated"] < 2000
    assert ref.counts()["map_size"] > 10000


# ---- bookkeeping across the 1024-point seam and LOST on a large map (test_gpu_map_capacity.py) ---------------------------------------------------------
from case_tables import MAPSEAM_RECIPES, RES_THREADS as BOOKKEEP_SMALL_MAX, mapseam_case     # noqa: E402


def _mapseam_rows(oracle_lib, name):
    prm, frames = mapseam_case(name)
    orc = oracle_lib.Oracle(prm, 1)
    rows = []
    for f in frames:
        orc.track_with_external_corners(*f)
        rows.append(dict(orc.counts(), status=orc.status))
    return prm, rows, orc


def test_mapseam_seam_matches_on_maps_either_side_of_1024_points(oracle_lib):
    """`seam`: the map at match time is 938, 1 043, 554, 533, 1 115, 1 102 points: from below k_track_mid's 1024-point threshold to above it, back (a cull
    of 591 points, taken by the large body, leaves a map for the small one) and above again; every frame TRACKING"""
    assert BOOKKEEP_SMALL_MAX == 1024
    prm, rows, _ = _mapseam_rows(oracle_lib, "seam")
    assert [r["status"] for r in rows] == [2] * len(rows) == [2] * len(MAPSEAM_RECIPES["seam"][1])
    at_match = [r["map_size_at_match"] for r in rows]
    assert at_match == [0, 938, 1043, 554, 533, 1115, 1102], at_match
    assert any(896 < m <= 1024 for m in at_match) and any(1024 < m <= 1152 for m in at_match)
    side = [m > 1024 for m in at_match[1:]]
    assert side == [False, True, False, False, True, True]                           # below, above, back, above
    assert all(r["n_matches"] >= 300 for r in rows[1:]) and all(r["overflow"] == 0 for r in rows)
    # both bodies compact: a cull on a map of either side, survivors and culled points in the hundreds
    assert [(r["map_size_at_match"] > 1024, r["n_culled"] > 90) for r in rows[2:]] == [(True, True), (False, True), (False, True), (True, True), (True, True)]


def test_mapseam_lost_goes_lost_on_a_map_of_more_than_1024_points(oracle_lib):
    """`lost`: three frames build a map of 1 420 points, the fourth shows nothing of the fixed strip: 16 matches after the doubled-radius pass, fewer than
    the 100 the recipe asks for -> LOST, with the bookkeeping applied where the points lie: nothing moves, hundreds of counters step; then the latch"""
    prm, frames = mapseam_case("lost")
    assert prm.min_num_matches_for_tracking == 100
    orc = oracle_lib.Oracle(prm, 1)
    rows, maps = [], []
    for f in frames:
        orc.track_with_external_corners(*f)
        rows.append(dict(orc.counts(), status=orc.status))
        maps.append(orc.map())
    assert [r["status"] for r in rows] == [2, 2, 2, 3, 3]
    lost = rows[3]
    assert lost["map_size_at_match"] == 1420 > BOOKKEEP_SMALL_MAX and lost["second_pass"] == 1 and 0 < lost["n_matches"] == 16 < prm.min_num_matches_for_tracking
    assert lost["map_size"] == 1420 and lost["n_culled"] == 0 and lost["n_triangulated"] == 0
    before, after = maps[2], maps[3]
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[3], after[3])           # positions and descriptors stay where they are
    assert (after[1] - before[1]).min() >= 0 and int((after[1] != before[1]).sum()) > 100        # counters of the visible, unmatched points
    assert int((after[2] - before[2]).sum()) == lost["n_matches"]                                # ages of the matched ones
    assert all(np.array_equal(a, b) for a, b in zip(maps[3], maps[4]))                           # LOST is sticky: nothing is computed


# ---- BRIEF at every seam of `inside` (test_gpu_brief_seams.py) -----------------------------------------------------------------------------------------
from case_tables import (BRIEF_BORDER, BRIEF_SEAM_DISP, BRIEF_SEAM_FRAMES, BRIEF_SEAM_H, BRIEF_SEAM_W, brief_seam_case, brief_seam_corners,      # noqa: E402
                         brief_seam_expected, brief_seam_tally)


def test_brief_seam_list_lands_on_every_seam(oracle_lib):
    """the corner list with the oracle alone: which corners brief_border_keep drops, where the others' centres lie, and that the oracle tracks the three frames"""
    W, H = BRIEF_SEAM_W, BRIEF_SEAM_H
    assert W % 64 == 0 and H % 2 == 1 and W - 40 >= BRIEF_BORDER and (W - 64) - 40 < BRIEF_BORDER         # the smallest multiple of 64 that holds the column list
    cl = brief_seam_corners()
    assert len(cl) == 65 and len(np.unique(cl, axis=0)) == 65
    for y in (33.0, 60.0):                                                                                # every integer column W - 40 .. W - 28 at two rows
        assert sorted(cl[cl[:, 1] == y][:, 0].tolist()) == [float(x) for x in range(W - 40, W - 27)]
    ties = {(x, y) for x, y in cl.tolist() if x % 1 == 0.5 or y % 1 == 0.5}
    assert {x for x, y in ties} >= {26.5, 27.5, 28.5, W - 29.5, W - 28.5, W - 27.5} and {y for x, y in ties} >= {26.5, 27.5, 28.5, H - 29.5, H - 28.5, H - 27.5}
    keep, cx, cy = brief_seam_expected(cl)
    # dropped by design: column W - 28 twice; 26.5 -> 26, W - 28.5 -> W - 28, W - 27.5 -> W - 28 (W even); 26.5 -> 26, H - 27.5 -> H - 28 (H odd).  Kept ties:
    # 27.5 -> 28 and 28.5 -> 28 (centres 28 and 29), W - 29.5 -> W - 30 (centre W - 29), H - 29.5 -> H - 30 (centre H - 29), H - 28.5 -> H - 29 (centre H - 28)
    dropped = {tuple(c) for c in cl[~keep].tolist()}
    assert dropped == {(W - 28.0, 33.0), (W - 28.0, 60.0), (26.5, 45.0), (W - 28.5, 53.0), (W - 27.5, 54.0), (44.0, 26.5), (68.0, H - 27.5)}, dropped
    t = brief_seam_tally(cl)
    assert t == dict(kept=58, left=3, top=3, right=5, bottom=3, below=4, overrun=12, slow_img=15, slow_plane=0, parity=[0, 1], quarter=[0, 1, 2, 3]), t
    assert min(t[k] for k in ("left", "top", "right", "bottom", "below", "overrun")) >= 3
    tr = brief_seam_tally(cl - [[float(BRIEF_SEAM_DISP), 0.0]])
    assert (tr["kept"], tr["below"], tr["overrun"], tr["slow_img"], tr["slow_plane"]) == (58, 4, 4, 8, 0), tr
    # the oracle keeps exactly those corners, in list order, and tracks the static scene on the map of its first frame
    prm, frames = brief_seam_case()
    assert len(frames) == BRIEF_SEAM_FRAMES == 3 and (prm.img_width, prm.img_height) == (W, H)
    orc = oracle_lib.Oracle(prm, 1)
    descs = []
    for i, f in enumerate(frames):
        orc.track_with_external_corners(*f)
        c = orc.counts()
        xy, _, d = orc.features(0)
        assert np.array_equal(xy, cl.astype(np.float32)[keep]) and c["n_left"] == c["n_right"] == t["kept"] and orc.status == 2, (i, c)
        assert i == 0 or c["n_matches"] >= 50, (i, c)
        descs.append(d)
    assert len(np.unique(descs[0], axis=0)) >= t["kept"] - 8          # (corners that share a centre share a descriptor)
    # a corner on the clipped path is not a degenerate one: its descriptor differs from that of the same centre one row up
    kept_c = cl[keep]
    below = np.flatnonzero(cy[keep] == H - 28)
    _, up = oracle_lib.brief(frames[0][0], (kept_c[below] - [[0.0, 1.0]]).astype(np.float32))
    assert len(up) == len(below) == 4 and all(not np.array_equal(a, b) for a, b in zip(up, descs[0][below]))


# ---- the domino scenes (test_gpu_resolver_chains.py) ----------------------------------------------------------------------------------------------
from case_tables import (DOMINO_BEST, DOMINO_MIN_DEPTH, DOMINO_OTHER, DOMINO_RATIO, DOMINO_SECOND, RES_LCAP, RES_THREADS, STAGED_CHAIN_DROPPED,
                         domino_scene, greedy_fixpoint, greedy_serial, map_lists, row_lists, super_chunks)


def test_fixpoint_equals_the_serial_scan_on_random_lists():
    """(a) == (b) on 400 random instances: few targets and distances from a small set (ties, contested targets, both branches of the accept rule,
    0 / 0), marks from before the call; and on a planted chain of n queries (b) needs exactly n + 1 iterations"""
    rng = np.random.default_rng(7)
    deep = 0
    for _ in range(400):
        nq, nt = int(rng.integers(1, 40)), int(rng.integers(1, 25))
        lists = []
        for q in range(nq):
            t = rng.choice(nt, size=int(rng.integers(0, min(nt, 6) + 1)), replace=False)
            lists.append(sorted((int(rng.choice([0, 10, 20, 24, 25, 30, 31, 60, 100])), int(k)) for k in t))
        marked = [int(k) for k in np.flatnonzero(rng.random(nt) < 0.15)]
        ratio = float(rng.choice([0.6, 0.8, 0.9]))
        a = greedy_serial(lists, ratio, 30.0, marked)
        b, it = greedy_fixpoint(lists, ratio, 30.0, marked)
        assert a == b and 1 <= it <= nq + 1, (lists, marked, ratio, a, b, it)
        assert len({d for d in a if d >= 0}) == sum(d >= 0 for d in a) and not set(a) & set(marked)
        deep = max(deep, it)
    assert deep >= 4
    for n in (1, 2, 17, 100):
        chain = [[(80, 0), (110, n)]] + [[(45, q - 1), (80, q), (110, n)] for q in range(1, n)]
        b, it = greedy_fixpoint(chain, 0.9, 30.0)
        assert b == list(range(n)) == greedy_serial(chain, 0.9, 30.0) and it == n + 1, (n, it)


def test_super_chunk_cut_is_the_resolvers():
    """the restated cut: QCAP queries, LCAP entries in lists rounded up to four, a list over KC alone"""
    assert super_chunks([5] * 5000) == [(0, 2048), (2048, 2048), (4096, 904)]
    assert super_chunks([45] * 600) == [(0, RES_LCAP // 48), (RES_LCAP // 48, 600 - RES_LCAP // 48)] and RES_LCAP // 48 == 512
    assert super_chunks([3, 129, 3, 0, 200]) == [(0, 1), (1, 1), (2, 2), (4, 1)]


def _triples(lists, chain):
    """(best, second, third) distances of the chain's queries behind its head, each as (min, median, max)"""
    a = np.array([[c[0] for c in lists[k][:3]] for k in chain[1:]])
    return [(int(a[:, j].min()), int(np.median(a[:, j])), int(a[:, j].max())) for j in range(3)]


_DOMINO = {}


def _domino_run(O, name):
    """the scene through the oracle alone, once per session: per frame its counts, status, row lists (frame 0) or map lists, the oracle's decisions and,
    for staged_chain's last frame, the staged lists with the marks find_matches left behind"""
    if name in _DOMINO:
        return _DOMINO[name]
    prm, frames, info = domino_scene(name)
    orc = O.Oracle(prm, 1)
    rows = []
    for i, f in enumerate(frames):
        (mxyz, _, _, mdesc), (sxyz, _, sdesc) = orc.map(), orc.staged()
        orc.track_with_external_corners(*f)
        fl, fr = orc.features(0), orc.features(1)
        row = dict(counts=orc.counts(), status=orc.status, row_pairs=orc.row_matches(), matches=orc.matches()[0])
        if i == 0:
            row["row_lists"] = row_lists(fl[0], fl[2], fr[0], fr[2], prm.img_height)
        else:
            row["map_lists"], vis = map_lists(prm, mxyz, mdesc, *orc.predicted_pose(), fl[0], fl[2])
            assert vis.all()
        if len(sxyz):
            row["staged_lists"], vis = map_lists(prm, sxyz, sdesc, *orc.pose(), fl[0], fl[2])
            assert vis.all()
        rows.append(row)
    _DOMINO[name] = (prm, info, rows)
    return _DOMINO[name]


def _map_conditions(prm, info, rows, frame):
    """find_matches of a frame: the oracle's matches are simulation (a)'s on lists built from its own features, map and predicted pose, every map point
    takes the feature of its own corner, and the oracle keeps tracking with all of them.  Returns the lists and (a)'s decisions."""
    r = rows[frame]
    lists = r["map_lists"]
    a = greedy_serial(lists, prm.tracking_ratio_test_threshold, prm.descriptor_matching_threshold)
    assert [d for d in a if d >= 0] == r["matches"].tolist()
    assert a == list(range(len(lists)))
    assert r["status"] == 2 and r["counts"]["n_matches"] == len(lists) >= info["n_chain"] and r["counts"]["second_pass"] == 0
    return lists, a


def test_map_chain_conditions(oracle_lib):
    """`map_chain`: 95 nodes + 5 spares, nothing lost at the border; frames 1 and 2 are one chain of 95 queries in one super-chunk, depth 96"""
    prm, info, rows = _domino_run(oracle_lib, "map_chain")
    n = info["n_chain"]
    assert n == 95 and info["n_corners"] == 100 and rows[0]["counts"]["n_triangulated"] == rows[0]["counts"]["map_size"] == 100
    for frame in (1, 2):
        lists, a = _map_conditions(prm, info, rows, frame)
        assert super_chunks([len(l) for l in lists]) == [(0, 100)] and max(len(l) for l in lists) == 5
        b, it = greedy_fixpoint(lists, prm.tracking_ratio_test_threshold, prm.descriptor_matching_threshold)
        assert b == a and it == 96 >= DOMINO_MIN_DEPTH["map_chain"] == 64
        # the chain itself: query i sees target i - 1, then target i, then an unrelated one, at the distances the patches were drawn for
        for k in range(1, n):
            (d1, t1), (d2, t2), (d3, _) = lists[k][:3]
            assert (t1, t2) == (k - 1, k) and DOMINO_BEST[0] <= d1 <= DOMINO_BEST[1] and DOMINO_SECOND[0] <= d2 <= DOMINO_SECOND[1] and d3 >= DOMINO_OTHER
        assert lists[0][0][1] == 0 and lists[0][1][0] >= DOMINO_OTHER
        assert _triples(lists, info["chain"]) == [(36, 47, 54), (70, 77, 86), (101, 117, 152)]
    # with room: the worst node stays 0.13 below the ratio threshold on the way in (best / second) and 0.04 on the way out (second / third)
    assert DOMINO_BEST[1] / DOMINO_SECOND[0] < 0.78 and DOMINO_SECOND[1] / DOMINO_OTHER <= 0.86 < DOMINO_RATIO == prm.tracking_ratio_test_threshold


def test_row_chain_conditions(oracle_lib):
    """`row_chain` = frame 0 of `map_chain`: row_match offers a query the 20 right features of its lattice row (19 nodes and the spare): five chains of
    19 running at once, depth 20; every left corner pairs with its own partner and triangulates"""
    prm, info, rows = _domino_run(oracle_lib, "map_chain")
    lists = rows[0]["row_lists"]
    assert [len(l) for l in lists] == [20] * 100
    a = greedy_serial(lists, prm.triangulation_ratio_test_threshold, prm.descriptor_matching_threshold)
    b, it = greedy_fixpoint(lists, prm.triangulation_ratio_test_threshold, prm.descriptor_matching_threshold)
    assert a == b == list(range(100)) and it == 20 >= DOMINO_MIN_DEPTH["row_chain"] == 16
    assert np.array_equal(rows[0]["row_pairs"], np.column_stack([np.arange(100), a]))
    heads = set(range(0, 95, 19))
    for k in range(95):
        if k not in heads:
            assert [t for _, t in lists[k][:2]] == [k - 1, k] and lists[k][2][0] >= DOMINO_OTHER
        else:
            assert lists[k][0][1] == k and lists[k][1][0] >= DOMINO_OTHER
    body = [k for k in range(95) if k not in heads]
    assert _triples(lists, [0] + body) == [(36, 47, 54), (70, 77, 86), (100, 108, 118)]


def test_chain_across_super_chunks_conditions(oracle_lib):
    """`chain_across_super_chunks`: 47 chain queries, 768 dense and 843 sparse fillers, 48 chain queries, 5 spares.  The dense fillers end super-chunk 0
    on the list area at query 610; the second half of the chain holds local queries 1000 .. 1047 of super-chunk 1, across local index 1 024; its head
    prefers the target of query 46, which carries super-chunk 0's permanent mark.  Depths 48 and 49."""
    prm, info, rows = _domino_run(oracle_lib, "chain_across_super_chunks")
    n, chain = info["n_chain"], info["chain"]
    half = n // 2
    assert (n, half, info["n_corners"]) == (95, 47, 1663) and rows[0]["counts"]["map_size"] == 1663
    for frame in (1, 2):
        lists, a = _map_conditions(prm, info, rows, frame)
        ncand = [len(l) for l in lists]
        chunks = super_chunks(ncand)
        assert chunks == [(0, 610), (610, 1053)] and max(ncand) == 45 <= 128
        assert sum((c + 3) & ~3 for c in ncand[:610]) <= RES_LCAP < sum((c + 3) & ~3 for c in ncand[:611])        # cut by the list area, among the dense fillers
        assert half < 610 < half + 768
        local = chain[half:] - 610
        assert local[0] == 1000 and local[-1] == 1047 and local[0] < RES_THREADS < local[-1] and np.array_equal(np.diff(local), np.ones(47))
        marked, depth = set(), []
        for b0, used in chunks:
            sub = lists[b0:b0 + used]
            b, it = greedy_fixpoint(sub, prm.tracking_ratio_test_threshold, prm.descriptor_matching_threshold, marked)
            assert b == a[b0:b0 + used]
            marked |= set(b)
            depth.append(it)
        assert depth == [48, 49] and depth[1] >= DOMINO_MIN_DEPTH["chain_across_super_chunks"] == 32
        head = lists[chain[half]]
        assert head[0][1] == chain[half - 1] < 610 and head[1][1] == chain[half]        # its best target was taken in super-chunk 0
        # without that mark the head would take it: the second half is decided wrongly from its first query on if the mark goes stale
        assert greedy_serial(lists[610:], prm.tracking_ratio_test_threshold, prm.descriptor_matching_threshold)[local[0]] == chain[half - 1]
        for j, k in enumerate(chain):
            if j:
                assert [t for _, t in lists[k][:2]] == [chain[j - 1], k] and lists[k][2][0] >= DOMINO_OTHER
    assert prm.img_width <= 4096 and prm.img_height <= 4096 and prm.detection_cell_size >= max(prm.img_width, prm.img_height)    # one detection cell


def test_staged_chain_conditions(oracle_lib):
    """`staged_chain`: frame 0 maps the 1 563 fillers, frame 1 stages the chain and the spares (100 points, in corner order), frame 2 runs them through
    update_staged: 97 promoted, the three spares whose corners are gone erased; the staged scan is one chain of 95, depth 96"""
    prm, info, rows = _domino_run(oracle_lib, "staged_chain")
    c = [r["counts"] for r in rows]
    assert prm.staged_threshold == 1 and all(r["status"] == 2 for r in rows)
    assert (c[0]["map_size"], c[0]["staged_size"]) == (1563, 0) and (c[1]["map_size"], c[1]["staged_size"], c[1]["n_matches"]) == (1563, 100, 1563)
    assert (c[2]["n_staged_promoted"], c[2]["n_staged_erased"], c[2]["staged_size"], c[2]["map_size"]) == (97, STAGED_CHAIN_DROPPED, 0, 1660)
    lists = rows[2]["staged_lists"]
    marks = rows[2]["matches"].tolist()              # what find_matches marked; nothing was culled
    assert len(lists) == 100 and c[2]["n_culled"] == 0 and len(marks) == 1563
    a = greedy_serial(lists, prm.tracking_ratio_test_threshold, prm.descriptor_matching_threshold, marks)
    b, it = greedy_fixpoint(lists, prm.tracking_ratio_test_threshold, prm.descriptor_matching_threshold, marks)
    assert a == b and it == 96 >= 16
    assert sum(d >= 0 for d in a) == c[2]["n_staged_promoted"] and sum(d < 0 for d in a) == c[2]["n_staged_erased"]
    assert a[:95] == info["chain"].tolist() and [d >= 0 for d in a[95:]] == [False] * STAGED_CHAIN_DROPPED + [True] * (5 - STAGED_CHAIN_DROPPED)


# ---- RGB-D at its depth and lens edges (test_gpu_rgbd_edges.py) ---------------------------------------------------------------------------------------
def _oracle_frame0(oracle_lib, case):
    orc = oracle_lib.Oracle(case["prm"], 2)
    g, _, f = case["frames"][0]
    orc.track_rgbd(g, f)
    return orc


def _assert_planted(oracle_lib, case, n_corners, n_kept):
    """the oracle keeps exactly the corners numpy float32 keeps, in list order, with their compute_features descriptors, and its map after frame 0 EQUALS
    the fp32 restatement of the back-projection"""
    assert len(case["xy"]) == n_corners and int(case["keep"].sum()) == n_kept
    orc = _oracle_frame0(oracle_lib, case)
    xy, _, desc = orc.features(0)
    k = case["keep"]
    assert orc.status == 2 and orc.counts()["n_left"] == n_kept and orc.counts()["n_right"] == 0
    assert np.array_equal(xy, case["xy"][k]) and np.array_equal(desc, case["desc"][k])
    mx, _, _, md = orc.map()
    assert np.array_equal(mx, rgbd_backproject(case["prm"], case["xy"][k], case["val"][k])) and np.array_equal(md, case["desc"][k])


def test_rgbd_planted_depth_classes(oracle_lib):
    """804 integer corners at distinct pixels, 15 classes of fp32 depth: NaN, the infinities, negatives, both zeros, a denormal and 3.4e38 are dropped,
    the two planes themselves are kept, one ulp outside them is dropped"""
    cls = rgbd_depth_classes()
    near, far = np.float32(RGBD_NEAR), np.float32(RGBD_FAR)
    assert cls.dtype == np.float32 and len(cls) == 15
    assert np.isnan(cls[0]) and cls[1] == np.inf and cls[2] == -np.inf and cls[3] == -1 and np.signbit(cls[4]) and cls[4] == 0 and not np.signbit(cls[5])
    assert 0 < cls[6] < np.finfo(np.float32).tiny and cls[14] > 3e38 and np.isfinite(cls[14])
    assert cls[7] < near == cls[8] < cls[9] and cls[11] < far == cls[12] < cls[13]
    assert np.nextafter(cls[7], far) == near and np.nextafter(cls[9], -far) == near and np.nextafter(cls[11], 2 * far) == far and np.nextafter(cls[13], near) == far
    case = rgbd_planted("f32")
    assert case["prm"].k1 == 0 and case["prm"].near_plane_distance == near and case["prm"].far_plane_distance == far
    plane = case["frames"][0][1]
    assert plane.dtype == np.float32 and np.array_equal(plane[case["xy"][:, 1].astype(int), case["xy"][:, 0].astype(int)], case["val"], equal_nan=True)
    which = np.arange(len(case["xy"])) % 15
    assert np.array_equal(case["keep"], (which >= 8) & (which <= 12)) and np.bincount(which, minlength=15).min() >= 53
    _assert_planted(oracle_lib, case, 804, 266)
    # the NaN class is what tells `d >= near && d <= far` from !(d < near) && !(d > far): the second form keeps every NaN corner
    with np.errstate(invalid="ignore"):
        assert int((~(case["val"] < near) & ~(case["val"] > far)).sum()) == 266 + int((which == 0).sum())
    # frames 1 - 3 (the world's own depth) go on TRACKING on the 266-point map
    orc = oracle_lib.Oracle(case["prm"], 2)
    for i, (g, _, f) in enumerate(case["frames"]):
        orc.track_rgbd(g, f)
        assert orc.status == 2 and (i == 0 or orc.counts()["n_matches"] > 150), (i, orc.counts())
    assert len(case["frames"]) == RGBD_PLANT_FRAMES == 4


@pytest.mark.parametrize("name", sorted(RGBD16_SETS))
def test_rgbd_planted_raws_decide_a_gate_by_rounding(oracle_lib, name):
    """a 16-bit set is worth its test only while ONE rounded fp32 multiply and a wider one fall on different sides of a plane at its pinned raw"""
    scale, raws = RGBD16_SETS[name]
    near, far = np.float32(RGBD_NEAR), np.float32(RGBD_FAR)
    assert scale.dtype == np.float32
    allr = np.arange(65536, dtype=np.uint16)
    p32 = allr.astype(np.float32) * scale
    p64 = allr.astype(np.float64) * np.float64(scale)         # exact: 16 x 24 significant bits
    assert p32.dtype == np.float32
    differ = np.flatnonzero(((p32 >= near) & (p32 <= far)) != ((p64 >= near) & (p64 <= far)))
    if name == "A":
        assert differ.tolist() == [2500] and p32[2500] == near and p64[2500] < near
        assert p32[25000] == far and p64[25000] < far and p32[2499] < near < p32[2501] and p32[24999] < far < p32[25001]
        kept = {2500, 2501, 12345, 24999, 25000}
    else:
        assert differ.tolist() == [5000] and p32[5000] == far and p64[5000] > far
        assert p32[500] == near and p64[500] > near and p32[499] < near < p32[501] and p32[4999] < far < p32[5001]
        # a division by the reciprocal scale, the other plausible conversion, moves raw 500 off the plane and raw 5000 beyond it
        div = allr.astype(np.float32) / (np.float32(1) / scale)
        assert div.dtype == np.float32 and div[500] > near and div[5000] > far
        kept = {500, 501, 4999, 5000}
    assert set(raws) >= kept | {0, 65535} and all((near <= p32[r] <= far) == (r in kept) for r in raws)
    # some kept raw's metres differ between the multiply and a division by the reciprocal scale: the map's exact z tells them apart
    dv = np.array(sorted(kept), np.float32) / (np.float32(1) / scale)
    assert (dv != p32[sorted(kept)]).any()
    case = rgbd_planted(name)
    u = case["frames"][0][1]
    ix, iy = case["xy"][:, 0].astype(int), case["xy"][:, 1].astype(int)
    assert u.dtype == np.uint16 and np.array_equal(u[iy, ix], np.array(raws, np.uint16)[np.arange(len(ix)) % len(raws)])
    assert np.array_equal(case["val"], u[iy, ix].astype(np.float32) * scale)
    n_kept = sum(len(range(j, 804, len(raws))) for j, r in enumerate(raws) if r in kept)
    _assert_planted(oracle_lib, case, 804, n_kept)
    orc = oracle_lib.Oracle(case["prm"], 2)
    for i, (g, _, f) in enumerate(case["frames"]):
        orc.track_rgbd(g, f)
        assert orc.status == 2, i


def test_rgbd_barrel_case_leaves_the_image(oracle_lib):
    """k1 < 0 on every frame: features kept outside [0, W) x [0, H), corners dropped for leaving the hash grid, and matches that land on the former"""
    world, prm = rgbd_world(RGBD_BARREL)
    assert prm.k1 < -1e-5
    all_valid = rgbd_world(dict(RGBD_BARREL, near_plane_distance=0.0, far_plane_distance=1e30))[1]
    orc = oracle_lib.Oracle(prm, 2)
    outside_matched, rows = 0, []
    for i in range(RGBD_BARREL_FRAMES):
        g, d = world.render_rgbd(i)
        orc.track_rgbd(g, d)
        c = orc.counts()
        xy = orc.features(0)[0]
        out = rgbd_outside(xy)
        # dropped by the grid rule: all corners minus the features of a frame whose depth is valid everywhere
        full = oracle_lib.Oracle(all_valid, 2)
        full.track_rgbd(g, np.ones_like(d))
        drops = len(oracle_lib.compute_features(g, prm)[0]) - full.counts()["n_left"]
        assert full.counts()["n_left"] == c["n_left"]          # (the world's depth is valid everywhere too)
        fi, _ = orc.matches()
        rows.append((c["n_matches"], int(out.sum()), drops, int(out[fi].sum()), float(xy[:, 0].max())))
        outside_matched += int(out[fi].sum())
        assert orc.status == 2 and (i == 0 or c["n_matches"] > 600), (i, c)
        assert out.sum() >= 5 and drops >= 5, (i, rows[-1])
        assert (xy[out, 0] < 650).all() and (xy[out, 1] < 500).all() and (xy >= 0).all()
    print(rows)
    assert outside_matched >= 1
    assert max(r[4] for r in rows) > 649


def test_rgbd_retry_case_runs_the_second_detection_pass(oracle_lib):
    world, prm = rgbd_world(RGBD_RETRY)
    orc = oracle_lib.Oracle(prm, 2)
    for i in range(RGBD_RETRY_FRAMES):
        orc.track_rgbd(*world.render_rgbd(i))
        c = orc.counts()
        assert c["retry_left"] == 1 and c["n_right"] == 0 and orc.status == 2 and 100 < c["n_left"] < 200, (i, c)
        assert i == 0 or c["n_matches"] > 100, (i, c)


@pytest.mark.parametrize("name", sorted(RGBD_NODEPTH))
def test_rgbd_frames_without_valid_depth(oracle_lib, name):
    prm, frames, status = rgbd_nodepth_script(name)
    orc = oracle_lib.Oracle(prm, 2)
    kinds = RGBD_NODEPTH[name][0]
    assert len(frames) == len(kinds) == len(status)
    for i, (g, handed, f) in enumerate(frames):
        assert f.dtype == np.float32 and handed.dtype == (np.uint16 if kinds[i] == "zero16" else np.float32)
        if kinds[i] != "world":
            with np.errstate(invalid="ignore"):
                assert not ((f >= np.float32(prm.near_plane_distance)) & (f <= np.float32(prm.far_plane_distance))).any()
            assert np.isnan(handed).all() if kinds[i] == "nan" else not handed.any()
        orc.track_rgbd(g, f)
        c = orc.counts()
        assert orc.status == status[i], (i, orc.status)
        if kinds[i] != "world":
            assert c["n_left"] == 0 and c["n_matches"] == 0, (i, c)
    if name == "nan_first":
        assert orc.counts()["map_size"] == 0
    else:
        assert orc.counts()["map_size"] > 1000


# ---- turns past 180 degrees: conditions on the inputs, the oracle alone ------------------------------------------------------------------------------
from case_tables import (MOTION_EDGE_CASES, MOTION_ONE, MOTION_RANDOM, MOTION_SMALL_ANGLES, TURN_CASES, TURN_CULLED_POINTS, TURN_KEEP_FRAMES,  # noqa: E402
                         TURN_KEEP_POINTS, TURN_MIN_ABS_W, behind_camera_in_image, motion_predict_longdouble, motion_slerp_dot, quat_to_R, turn_case)

_TURNS = {}


def _turn_run(name):
    """one oracle run per case, shared by the guards: per frame the status, the pose, the predicted pose (None for a frame that made none) and the number
    of map points at match time that the near plane alone keeps out (with the gate as it is, and restated without the comparison)"""
    if name not in _TURNS:
        from oracle import pyoracle as O
        world, prm, sensor, n = turn_case(name)
        orc = O.Oracle(prm, sensor)
        rows = []
        for i in range(n):
            at_match = orc.map()[0]
            if sensor == 1:
                orc.track(*world.render_stereo(i))
            else:
                orc.track_rgbd(*world.render_rgbd(i))
            q, p = orc.pose()
            pred, behind, ungated = None, 0, 0
            if orc.counts()["map_size_at_match"] > 0:
                assert orc.counts()["map_size_at_match"] == len(at_match)
                pred = orc.predicted_pose()
                behind = behind_camera_in_image(prm, at_match, pred[0], pred[1])
                ungated = behind_camera_in_image(prm, at_match, pred[0], pred[1], near_gate=False)
            rows.append(dict(status=orc.status, q=q, p=p, pred=pred, behind=behind, ungated=ungated))
        _TURNS[name] = (world, prm, rows)
    return _TURNS[name]


def test_turn_worlds_are_functions_of_their_seed():
    """the same frame from two instances, another one from another seed; the room's depth is the planar depth of what the gray image shows"""
    from parity_util import make_case
    from turn_worlds import RolledWorld, RoomWorld
    base, _, _ = make_case("kitti", 0, 0.25)
    cam = (base.W, base.H, base.fx, base.fy, base.cx, base.cy, base.baseline)
    a, b, c = RoomWorld(*cam, seed=3), RoomWorld(*cam, seed=3), RoomWorld(*cam, seed=4)
    for i in (0, 40, 77):
        assert all(np.array_equal(x, y) for x, y in zip(a.render_stereo(i), b.render_stereo(i)))
        assert not np.array_equal(a.render_stereo(i)[0], c.render_stereo(i)[0])
    g, d = a.render_rgbd(40)
    assert np.array_equal(g, a.render_stereo(40)[0]) and d.dtype == np.float32 and d.min() > 1.0 and d.max() < 30.0
    assert a.render_stereo(40) is a.render_stereo(40)                                        # frames are kept
    R, t = a.pose(72)                                                                        # 180 degrees of yaw: the far side of the circle, looking back
    assert np.allclose(R, np.diag([-1.0, 1, -1]), atol=1e-12) and np.allclose(t[[0, 2]], [6.0, 0.0], atol=1e-12)
    r1, r2 = RolledWorld(base, 3.0), RolledWorld(base, 3.0)
    assert all(np.array_equal(x, y) for x, y in zip(r1.render_stereo(30), r2.render_stereo(30)))
    R30, t30 = r1.pose(30)
    Rb, tb = base.pose(30)                                                                   # (the wrapped world keeps its own trajectory)
    c90 = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    assert np.allclose(R30, Rb @ c90, atol=1e-12) and np.array_equal(t30, tb)


@pytest.mark.parametrize("name", sorted(TURN_CASES))
def test_turn_case_conditions(oracle_lib, name):
    """every frame TRACKING; |w| of every pose at least 1e-3 (the sign k_pnp publishes is then no matter of rounding); the pose flips (q . previous q < 0) and a
    prediction with w < 0 follows a pose with w >= 0; the rotation leaves the identity far enough for R[0] < 0"""
    _, prm, rows = _turn_run(name)
    assert [r["status"] for r in rows] == [2] * len(rows), [i for i, r in enumerate(rows) if r["status"] != 2]
    w = np.array([r["q"][0] for r in rows])
    print(f"{name}: min |w| {np.abs(w).min():.4f} at frame {int(np.abs(w).argmin())}")
    assert np.abs(w).min() >= TURN_MIN_ABS_W and w.min() >= 0.0
    neg = [(i, float(r["pred"][0][0])) for i, r in enumerate(rows) if r["pred"] is not None and r["pred"][0][0] < 0 and r["q"][0] >= 0]
    flips = [i for i in range(1, len(rows)) if rows[i]["q"] @ rows[i - 1]["q"] < 0]
    print(f"{name}: predicted w < 0 at {neg}, pose flips at {flips}")
    assert neg and flips
    assert min(quat_to_R(r["q"])[0, 0] for r in rows) < -0.9


def test_room_loop_keep_has_points_behind_the_camera_inside_the_image(oracle_lib):
    """with culling off, on at least 100 frames at least 100 map points at match time lie behind the camera under the predicted pose and project inside the
    image: is_point_visible's `cz < near_plane` alone keeps them out of the lists.  Restated without that comparison the count is zero on every frame; under
    the default culling (room_loop) there is never more than a handful."""
    _, _, rows = _turn_run("room_loop_keep")
    behind = np.array([r["behind"] for r in rows])
    print(f"room_loop_keep: {int((behind >= TURN_KEEP_POINTS).sum())} frames with {TURN_KEEP_POINTS}+ such points, peak {behind.max()}")
    assert (behind >= TURN_KEEP_POINTS).sum() >= TURN_KEEP_FRAMES
    assert not any(r["ungated"] for r in rows)
    _, _, rows = _turn_run("room_loop")
    assert max(r["behind"] for r in rows) <= TURN_CULLED_POINTS, max(r["behind"] for r in rows)


def test_motion_table_takes_every_branch():
    """MOTION_EDGE_CASES: both arms of |d| >= one among the small angles (and the threshold between 2e-8 and 5e-8), d < 0, d = +0.0, a zero inverse, scaled
    and unnormalised quaternions, and the random rows' d of both signs"""
    d = {lab: motion_slerp_dot(st, q) for lab, st, q, _ in MOTION_EDGE_CASES}
    assert len(d) == len(MOTION_EDGE_CASES) and sum(lab.startswith("random_") for lab in d) == MOTION_RANDOM
    assert d["stationary"][0] == 1.0
    small = [d[f"small_{a:g}"][0] for a in MOTION_SMALL_ANGLES]
    assert any(x >= MOTION_ONE for x in small) and any(x < MOTION_ONE for x in small)
    assert d["small_2e-08"][0] >= MOTION_ONE > d["small_5e-08"][0]
    for a in MOTION_SMALL_ANGLES:
        assert d[f"small_{a:g}_negated_velocity"][0] == -d[f"small_{a:g}"][0] == d[f"small_{a:g}_negated_pose"][0]
    for lab in ("orthogonal_axes", "orthogonal_cancelling"):
        assert d[lab][0] == 0.0 and not np.signbit(d[lab][0])
    assert abs(d["wide_90"][0]) < 1e-15 and -1.0 < d["wide_179"][0] < -0.999 and d["wide_179.999"][0] < -0.9999999 and d["wide_179.999"][0] > -MOTION_ONE
    assert d["zero_last_q"] == (0.0, 0.0)
    assert abs(d["last_q_norm_3"][1] - 1 / 3) < 1e-12 and abs(d["last_q_norm_1e-3"][1] - 1e3) < 1e-9 and abs(d["cur_q_norm_2"][1] - 2) < 1e-12
    rnd = np.array([d[f"random_{k}"][0] for k in range(MOTION_RANDOM)])
    assert (rnd < 0).sum() > 50 and (rnd > 0).sum() > 50 and (np.abs(rnd) < MOTION_ONE).all()


def test_oracle_motion_model_equals_the_longdouble_restatement(oracle_lib):
    """the oracle's lvto_motion_predict on the whole table against lvt_motion_model.cpp:42-65 restated in numpy.longdouble (64-bit significand): the reference
    is pinned before the GPU tier uses it as one.
      copies (next[0..3] = q, next[8..10] = p): bit-equal.
      quaternions (next[4..7], q_out; components <= 1): the path is about 20 roundings of 1.1e-16 on quantities <= 1 (2.3e-15) plus acos and two sin within an
      ulp; 1e-14 leaves a factor of four.
      positions (next[11..13], p_out): three roundings on quantities up to 2 M, M = the largest position / velocity component: 4 eps M."""
    assert np.finfo(np.longdouble).eps < 1e-18, "numpy.longdouble is no wider than double here: the restatement would pin nothing"
    worst_q = worst_p = 0.0
    for lab, st, q, p in MOTION_EDGE_CASES:
        nx, qo, po = oracle_lib.motion_predict(st, q, p)
        ln, lq, lp = motion_predict_longdouble(st, q, p)
        assert np.array_equal(nx[0:4], q) and np.array_equal(nx[8:11], p), lab
        eq = float(max(np.abs(qo - lq).max(), np.abs(nx[4:8] - ln[4:8]).max()))
        M = float(np.abs(np.concatenate([st[8:14], p])).max())
        ep = float(max(np.abs(po - lp).max(), np.abs(nx[11:14] - ln[11:14]).max())) / M
        worst_q, worst_p = max(worst_q, eq), max(worst_p, ep)
        assert eq <= 1e-14, f"{lab}: quaternion differs by {eq:.3e}"
        assert ep <= 4 * np.finfo(np.float64).eps, f"{lab}: position differs by {ep:.3e} relative"
        assert abs(float((qo * qo).sum()) - 1) < 1e-15 and abs(float((nx[4:8] * nx[4:8]).sum()) - 1) < 1e-15, lab
    print(f"oracle vs longdouble: quaternions {worst_q:.3e}, positions {worst_p:.3e} relative")


# ---- the batched Hamming matcher's instances and bounds (test_gpu_hamming_instances.py): the table and the constructed inputs, no GPU ---------------------
from case_tables import (HAMMING_CHUNKED_GRID, HAMMING_CHUNKED_ROW, HAMMING_COUNT_GEOMETRY, HAMMING_COUNT_KS, HAMMING_FAMILIES, HAMMING_GEOMETRY,  # noqa: E402
                         HAMMING_INSTANCE_CASES, HAMMING_PACKED_LAYOUTS, HAMMING_R2_BOUNDARIES, HAMMING_RING_OFFSETS, HAMMING_RING_QUERIES, HB_LDS_MAX,
                         HB_MASK_BITS, HB_MMAX, HB_NMAX, HB_RANGE_MAX, HB_STATIC_LDS, HB_THREADS, HB_TWO_STAGE_MAX, hamming_admitted,
                         hamming_boundary_problem, hamming_chunked_grid_case, hamming_chunked_row_case, hamming_count_case, hamming_count_check,
                         hamming_csr, hamming_grid, hamming_instance, hamming_instance_problem, hamming_lds_bytes, hamming_nbins, hamming_packed_starts_case,
                         hamming_packed_words, hamming_phantom_case, hamming_scan_chunk, hamming_window_counts)


def test_hamming_table_reaches_every_admissible_instance():
    """the table's instances are ALL the instances a launch can reach on its geometry: 4 families x 15 (QPT, TPT) classes; (4, 4) is out because its
    smallest member, M = N = 3073, needs 42 N + 14 M = 172 088 bytes of LDS, more than a workgroup's 163 840 -- and for no other reason"""
    rows, cols = HAMMING_GEOMETRY
    reached = set()
    for fam, q, t, member, M, N in HAMMING_INSTANCE_CASES:
        mode, nsp, r2 = HAMMING_FAMILIES[fam]
        assert hamming_admitted(mode, M, N, rows, cols), (fam, M, N)
        assert hamming_instance(mode, r2, M, N) == (mode, nsp, q, t), (fam, M, N)
        reached.add((mode, nsp, q, t))
        if member == "smallest":
            assert (M, N) == (HB_THREADS * (q - 1) + 1, HB_THREADS * (t - 1) + 1)
        else:        # nothing larger in its class launches: M or N is at the class's end, or one more of it is refused
            assert M == HB_THREADS * q or not hamming_admitted(mode, M + 1, N, rows, cols)
            assert N == HB_THREADS * t or not hamming_admitted(mode, M, N + 1, rows, cols)
            assert M == HB_THREADS * q or N == HB_THREADS * (t - 1) + 1
    admissible = set()
    for fam, (mode, nsp, r2) in HAMMING_FAMILIES.items():
        for q in range(1, 5):
            for t in range(1, 5):
                if hamming_admitted(mode, HB_THREADS * (q - 1) + 1, HB_THREADS * (t - 1) + 1, rows, cols):      # the class's cheapest member
                    admissible.add((mode, nsp, q, t))
    assert reached == admissible and len(reached) == 60 and len(HAMMING_INSTANCE_CASES) == 120
    assert {(1, 1), (0, 3), (0, 5), (0, 0)} == {i[:2] for i in reached}
    for fam, (mode, nsp, r2) in HAMMING_FAMILIES.items():
        assert (mode, nsp, 4, 4) not in reached
        assert HB_MMAX >= 3073 and HB_NMAX >= 3073                                    # not the caps ...
        assert hamming_lds_bytes(3073, 3073, 0) == 42 * 3074 + 14 * 3074 - 40 * 1 - 12 * 1 + 4 + 16 > HB_LDS_MAX   # ... the carve-up alone, without a single bin
    assert [hamming_csr(HAMMING_FAMILIES[f][2]) for f in ("csr1", "csr2", "any")] == [1, 2, 3]
    assert hamming_lds_bytes(1500, 1000, 800) == 42 * 1500 + 14 * 1000 + 4 * 801 + 16 and HB_STATIC_LDS == 128 + 256 + 4 + 12


def test_hamming_instance_problems_take_their_branches():
    """the largest member of every class: problem 1's cluster pushes windows past 64 candidates and ranges past 63 (the in-place fallbacks), problem 0
    has windows the masks hold, flags, ties and queries outside the image; in row mode only problem 1 has rows that are no in-range integers"""
    rows, cols = HAMMING_GEOMETRY
    for fam, q, t, member, M, N in HAMMING_INSTANCE_CASES:
        if member != "largest":
            continue
        mode, nsp, r2 = HAMMING_FAMILIES[fam]
        qd, qxy, td, txy, tf = hamming_instance_problem(fam, M, N)
        assert qd.shape == (2, M, 32) and td.shape == (2, N, 32) and 0.1 < tf.mean() < 0.2
        assert len(np.unique(td[0], axis=0)) == 8 and len(np.unique(td[1], axis=0)) > N // 2
        o = qxy[0]
        assert (o[:, 0] < 0).any() and (o[:, 0] > cols).any() and (o[:, 1] < 0).any() and (o[:, 1] > rows).any()
        if mode == 1:
            is_row = lambda y: (y == np.floor(y)) & (y >= 0) & (y <= rows)
            assert is_row(txy[0, :, 1]).all() and (~is_row(txy[1, tf[1] == 0, 1])).sum() >= 5 and np.isnan(txy[1, :, 1]).sum() == 1
            continue
        csr = hamming_csr(r2)
        w0, w1 = (hamming_window_counts(qxy[b], txy[b], tf[b], csr, rows, cols) for b in (0, 1))
        assert (w1.sum(axis=1) > HB_TWO_STAGE_MAX).sum() >= 10 and (w1.max(axis=1) > HB_RANGE_MAX).sum() >= 10, (fam, M, N)
        w = np.vstack([w0, w1])
        total = w.sum(axis=1)
        if nsp == 3:       # both mask words, the in-place walk of a packed query (total past MASK_BITS), and of one whose ranges do not fit
            fits = w.max(axis=1) <= HB_RANGE_MAX
            assert (fits & (total <= 32)).sum() >= 10 and (fits & (total > 32) & (total <= HB_MASK_BITS)).sum() >= 3 and (fits & (total > HB_MASK_BITS)).sum() >= 3, (fam, M, N)
        if nsp == 5:
            assert (total <= 32).sum() >= 10 and ((total > 32) & (total <= HB_TWO_STAGE_MAX)).sum() >= 10, (fam, M, N)


@pytest.mark.parametrize("csr", [1, 2])
def test_hamming_count_populations_hold_their_counts(csr):
    """binned with floor(x / 25) in fp32, every query of a population sees exactly its k window candidates, range by range"""
    stats = hamming_count_check(csr)
    ks = sorted({k for k, _, _, _ in stats})
    assert ks == sorted(HAMMING_COUNT_KS + (66,)) and {31, 32, 33, 40, 41, 42, 63, 64, 65} <= set(ks)
    assert {HB_MASK_BITS, HB_MASK_BITS + 1, HB_RANGE_MAX, HB_RANGE_MAX + 1, HB_TWO_STAGE_MAX, HB_TWO_STAGE_MAX + 1, 32, 33} <= set(ks)
    if csr == 1:     # a single range of 63 and of 64, in either layout
        longest = {(layout, longest) for _, layout, longest, _ in stats}
        assert {("one", 63), ("one", 64), ("split", 63), ("split", 64)} <= longest
    assert sum(n_exact for _, _, _, n_exact in stats) >= 20
    assert hamming_nbins(0, *HAMMING_COUNT_GEOMETRY) + 1 <= HB_THREADS


def test_hamming_boundary_problem_sits_on_the_circles():
    """the r2 list switches the family where it says, and the ring features lie at distance^2 0, 625 and 2500 EXACTLY in fp32: accepted or rejected by
    the strict comparison alone"""
    from hamming_util import radius_mask
    assert [f for _, f in HAMMING_R2_BOUNDARIES] == ["csr1", "csr1", "csr1", "csr2", "csr2", "any", "any"]
    r2s = [r for r, _ in HAMMING_R2_BOUNDARIES]
    assert all(r.dtype == np.float32 for r in r2s) and r2s[3] > np.float32(625) and r2s[3] - np.float32(625) < 1e-4 and r2s[5] - np.float32(2500) < 3e-4
    for r2, fam in HAMMING_R2_BOUNDARIES:
        assert hamming_instance(0, r2, 600, 1200)[:2] == HAMMING_FAMILIES[fam][:2]
    assert [hamming_csr(r) for r in r2s] == [1, 1, 1, 2, 2, 3, 8]
    qd, qxy, td, txy, tf = hamming_boundary_problem()
    n25 = sum(1 for x, y in HAMMING_RING_OFFSETS if x * x + y * y == 625)
    n50 = sum(1 for x, y in HAMMING_RING_OFFSETS if x * x + y * y == 2500)
    assert (n25, n50, len(HAMMING_RING_OFFSETS)) == (8, 6, 15)
    for b in range(2):
        q, t = qxy[b, :HAMMING_RING_QUERIES], txy[b]
        dx, dy = t[None, :, 0] - q[:, None, 0], t[None, :, 1] - q[:, None, 1]
        d2 = (dx * dx + dy * dy).astype(np.float32)
        assert d2.dtype == np.float32
        assert ((d2 == 0).sum(axis=1) >= 1).all() and ((d2 == 625).sum(axis=1) >= n25).all() and ((d2 == 2500).sum(axis=1) >= n50).all()
        # what the switch of the family must not change: 625 admits nothing new at distance 25, its successor admits all eight
        m = [radius_mask(q, t, r) for r in r2s]
        assert not (m[0] & (d2 == 0)).any() and (m[1] & (d2 == 0)).sum() >= HAMMING_RING_QUERIES
        assert not (m[2] & (d2 == 625)).any() and ((m[3] & (d2 == 625)).sum(axis=1) >= n25).all()
        assert not (m[4] & (d2 == 2500)).any() and ((m[5] & (d2 == 2500)).sum(axis=1) >= n50).all()


def test_hamming_chunked_cases_fill_every_chunk():
    """the sizes sit on either side of the scan's threshold, and every chunk of the chunked scan that holds a bin holds a feature"""
    assert [hamming_scan_chunk(r + 1) for r in HAMMING_CHUNKED_ROW] == [0, 2, 2, 3]
    assert [hamming_nbins(1, r, 0) + 1 for r in HAMMING_CHUNKED_ROW] == [1024, 1025, 1026, 2162]
    for rows in HAMMING_CHUNKED_ROW:
        qd, qxy, td, txy, tf, cols = hamming_chunked_row_case(rows)
        chunk = max(hamming_scan_chunk(rows + 1), 1)
        assert not tf[0].any() and 0.05 < tf[1].mean() < 0.15
        for b in range(2):
            y = txy[b, tf[b] == 0, 1]
            if b == 0:
                assert {0, 1, rows - 1, rows} <= set(y.tolist())
                assert set(range(-(-(rows + 1) // chunk))) == set((y.astype(int) // chunk).tolist())
            assert (qxy[b, :, 1] < 2).any() and (qxy[b, :, 1] > rows).any()
        assert (txy[0, :, 1] == np.floor(txy[0, :, 1])).all() and (txy[1, :, 1] != np.floor(txy[1, :, 1])).sum() > 100
        assert hamming_admitted(1, qd.shape[1], td.shape[1], rows, cols)
    assert {(r, c) for r, c, _ in HAMMING_CHUNKED_GRID} == {(1200, 4096), (1000, 2600)}
    assert [HAMMING_FAMILIES[f][1] for f in ("csr1", "csr2", "any")] == [3, 5, 0]
    assert sorted({hamming_instance(0, r2, 700, 1300)[1] for _, _, r2 in HAMMING_CHUNKED_GRID}) == [0, 3, 5]
    for rows, cols in ((1200, 4096), (1000, 2600)):
        nbx, nby = hamming_grid(0, rows, cols)
        nbins = nbx * nby
        chunk = hamming_scan_chunk(nbins)
        assert (nbx, nby) in ((164, 48), (104, 40)) and chunk in (8, 5) and (nbins + 1) % chunk == 1
        qd, qxy, td, txy, tf = hamming_chunked_grid_case(rows, cols)
        assert 1000 < td.shape[1] <= 1500 and hamming_admitted(0, qd.shape[1], td.shape[1], rows, cols)
        for b in range(2):
            t = txy[b]
            bins = np.floor(t[:, 1] / np.float32(25)).astype(int) * nbx + np.floor(t[:, 0] / np.float32(25)).astype(int)
            assert bins.min() >= 0 and bins.max() == nbins - 1
            assert set(range(-(-nbins // chunk))) == set((bins // chunk).tolist())              # (flagged or not: the scan adds every chunk's counts)
            assert len({int(x) % chunk for x in bins}) == chunk                                 # ... at every place inside a chunk
            last_col = np.floor(qxy[b, :, 0] / np.float32(25)) >= nbx - 2
            assert last_col.sum() >= 50 and (qxy[b, :, 0] > cols).any() and (qxy[b, :, 1] > rows).any() and (qxy[b] < 0).any()
            w = hamming_window_counts(qxy[b], txy[b], tf[b], 1, rows, cols)
            assert (w[last_col].sum(axis=1) > 0).sum() >= 30                                    # windows at the end of a cell row that hold candidates


def test_hamming_packed_start_layouts_reach_2048():
    """without a flag and with N = 2048 the layouts hold queries whose range starts ARE 2048: all three (`behind`), or the two behind a first range that
    ends at the last feature, of even length in problem 0 and odd in problem 1 (`tail`); the control has none"""
    rows, cols = HAMMING_GEOMETRY
    assert HAMMING_PACKED_LAYOUTS == ("behind", "tail", "control")
    for layout in HAMMING_PACKED_LAYOUTS:
        qd, qxy, td, txy, tf = hamming_packed_starts_case(layout)
        assert not tf.any() and td.shape[1] == (2047 if layout == "control" else 2048) and hamming_instance(0, 625.0, qd.shape[1], td.shape[1]) == (0, 3, 1, 2)
        for b in range(2):
            W0, W1, s, l = hamming_packed_words(qxy[b], txy[b], rows, cols)
            packed = W0 != 0xFFFFFFFF
            if layout == "control":
                assert s.max() == 2047
                continue
            if layout == "behind":
                assert (packed & (s == 2048).all(axis=1)).sum() >= 100
                assert (packed & (s[:, 0] < 2048) & (l[:, 0] > 0) & (s[:, 1] == 2048)).sum() >= 10
            else:
                at_end = packed[:100] & (s[:100, 0] + l[:100, 0] == 2048) & (l[:100, 0] > 0) & (s[:100, 1] == 2048) & (s[:100, 2] == 2048)
                assert at_end.sum() >= 60
                assert set((l[:100, 0][at_end] % 2).tolist()) == {b}
            # what the 11-bit fields make of such a start: the decoded ranges differ from the true ones
            dec_l0 = W0[packed] >> 22
            assert (dec_l0 != l[packed, 0]).any() or (((W1[packed] >> 11) & 63) != l[packed, 1]).any()


def test_hamming_phantom_case_decodes_inside_a_circle():
    """the slot words of the constructed input, modelled: query 0's words, read as coordinates once its mask is stored, lie inside Q's circle; Q's first
    range ends at feature 2048 with an even length and the starts behind it are 2048; the sorted order puts query 0 at slot 960 and Q at slot 1088"""
    rows, cols = HAMMING_GEOMETRY
    qd, qxy, td, txy, tf, info = hamming_phantom_case()
    qxy, txy = qxy[0], txy[0]
    assert txy.shape == (2048, 2) and not tf.any() and hamming_instance(0, 625.0, len(qxy), 2048) == (0, 3, 2, 2)
    W0, W1, s, l = hamming_packed_words(qxy, txy, rows, cols)
    Q = info["Q"]
    assert s[Q].tolist() == [2046, 2048, 2048] and l[Q].tolist() == [2, 0, 0] and W0[Q] != 0xFFFFFFFF
    assert (int(W0[Q]) >> 22, int(W0[Q]) & 2047) == (3, 2046)                           # decoded: one candidate more, at position 2046 + 2 = N
    assert s[0].max() < 2048 and l[0].tolist() == [20, 19, 1]
    # query 0's candidates in flattened order, cell by cell; inside a cell the order is the scatter's, so a cell must be all in or all out
    from hamming_util import radius_mask
    nbx = hamming_grid(0, rows, cols)[0]
    cell = np.floor(txy[:, 1] / np.float32(25)).astype(int) * nbx + np.floor(txy[:, 0] / np.float32(25)).astype(int)
    inside = radius_mask(qxy[:1], txy, 625.0)[0]
    bits = []
    for cy, cx in [(0, 9), (0, 10), (0, 11), (1, 9), (1, 10), (1, 11), (2, 9), (2, 10), (2, 11)]:
        k = np.flatnonzero(cell == cy * nbx + cx)
        if cy > 0:
            assert len(set(inside[k].tolist())) <= 1
        bits += inside[k].tolist()
    assert len(bits) == 40 <= HB_MASK_BITS
    hi = sum(int(v) << i for i, v in enumerate(bits[32:]))
    assert hi == 0b10000110
    W1_after = (int(W1[0]) & 0x7FFFFF) | (hi << 23)
    phantom = np.array([W0[0], W1_after], np.uint32).view(np.float32)
    assert 0 <= phantom[0] < 1e-28 and 130.0 < phantom[1] < 131.0
    assert radius_mask(qxy[Q:Q + 1], phantom[None, :], 625.0)[0, 0] and not radius_mask(qxy[Q:Q + 1], txy, 625.0).any()
    # the order of stage 4a: classes by min(window candidates, 63), heaviest first
    total = l.sum(axis=1)
    assert (total[info["heavy"]] > 41).all() and len(info["heavy"]) == 960 and (total[info["medium"]] == 30).all() and len(info["medium"]) == 127
    assert total[0] == 40 and total[Q] == 2 and (total[info["light"]] == 0).all()
    assert (total > total[0]).sum() == 960 and (total > total[Q]).sum() == 1088 >= HB_THREADS + 64
    # no other query's own words are touched by a start of 2048, except the ten far below (their extra candidates are features of rows 0: out of reach)
    others = np.concatenate([info["heavy"], info["medium"]])
    assert s[others].max() < 2048
