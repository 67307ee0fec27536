"""The planted cases of the candidate-list tests: tests/test_list_cases.py (CPU tier: the oracle alone shows that every case still plants what it claims)
and tests/test_gpu_candidate_lists.py (-m gpu: both list builders against tests/lists_util.py on these cases).

Features come through track_with_external_corners: the positions are the case's own (fractional where a case wants it), the descriptors are BRIEF on a
seeded noise image, so unrelated features lie about 128 +- 8 bits apart and equal distances -- with them the index tie rule -- occur by themselves;
duplicate corners (identical coordinates) give ties at every distance.  Only corners with cvRound(x) in [28, W - 28) and cvRound(y) in [28, H - 28) survive
BRIEF's border filter, in the order they were given.  That is why the row band's clips at 0 and at H cannot be planted: no feature lies within 2 rows of
either, so max(int(y) - 2, 0) and min(int(y) + 2, H) never bind.  They are not faked.

Row cases (ROW_CASES): ONE frame on a fresh stereo handle; row lists are built for every left feature on every frame, the first included.
Map cases (MAP_CASES): a static camera in front of a noise wall at 10 m, three frames.  Frame 0 triangulates every corner of P0, frame 1 adds the corners P1
(triangulated behind the early part: on frame 2 they are the late part, listed by k_match_map), and frame 2's left corners are planted around the frame-0
corners, whose positions are the map points' nominal projections under the static camera.

A case is a dict: prm, frames [(left, right, corners_left, corners_right)], env (what the handle is created under, beside LVT_AMD_BINNED_LISTS), plants (text),
claims (what the reference over the case's own inputs must show; `check_*_claims` asserts them, on the oracle's features in the CPU tier and on the
device's in the GPU tier) and expect (the info record: stood-down flags, pass 2)."""
import functools

import numpy as np

import lvt_amd
import lists_util as LU

f32 = np.float32
BORDER = 28
DISP = 8                       # px: the right eye is the left one moved 8 px (z = fx * baseline / 8)
LS_NMAX, LS_BINS = 1536, 1100  # k_lists.hip: the binned kernel stands down above these (train features / bins)


def below(v):
    return float(np.nextafter(f32(v), f32(-np.inf)))


def above(v):
    return float(np.nextafter(f32(v), f32(np.inf)))


def survivors(corners, W, H):
    """the corners BRIEF keeps, as the fp32 pairs the feature arrays hold, in order (cvRound: to nearest, halves to even)"""
    c = np.asarray(corners, np.float64).reshape(-1, 2).astype(f32)
    rx, ry = np.rint(c[:, 0]), np.rint(c[:, 1])
    return c[(rx >= BORDER) & (rx < W - BORDER) & (ry >= BORDER) & (ry < H - BORDER)]


@functools.lru_cache(maxsize=None)
def noise_pair(W, H, seed=7):
    rng = np.random.default_rng([seed, W, H])
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    return left, np.ascontiguousarray(np.roll(left, -DISP, axis=1))


def row_params(W, H):
    return lvt_amd.kitti_params(width=W, height=H, fx=300.0, fy=300.0, cx=W / 2.0, cy=H / 2.0, baseline=0.5)


def scatter(rng, n, W, H, x0=BORDER, y0=BORDER, x1=None, y1=None):
    """n distinct integer positions inside the border"""
    x1, y1 = (W - BORDER if x1 is None else x1), (H - BORDER if y1 is None else y1)
    cells = rng.permutation((x1 - x0) * (y1 - y0))[:n]
    assert len(cells) == n
    return np.column_stack([x0 + cells % (x1 - x0), y0 + cells // (x1 - x0)]).astype(np.float64)


# ================================================================================================================================================================
# row cases
# ================================================================================================================================================================
def _row_case(name, W, H, cl, cr, plants, claims=None, expect=None, env=None):
    left, right = noise_pair(W, H)
    return dict(name=name, kind="row", W=W, H=H, prm=row_params(W, H), frames=[(left, right, np.asarray(cl, np.float64).reshape(-1, 2), np.asarray(cr, np.float64).reshape(-1, 2))],
                plants=plants, claims=claims or {}, expect=dict({"stood_down_row": 0}, **(expect or {})), env=env or {})


def _band(c, total, x0=30, step=3):
    """`total` right features of the band [c - 2, c + 2]: rows c - 2 .. c + 2 in turn"""
    return [[x0 + step * (i // 5) + (i % 5) * 0.25, c - 2 + i % 5] for i in range(total)]


def row_band_edges():
    W, H = 320, 400
    cl = [[100, 80.0], [104, 80.9]] + [[60 + 9 * i, 150 + 20 * (i % 7)] for i in range(20)]
    edge = [[60, 78.0], [61, below(78)], [62, 82.0], [63, above(82)], [64, 82.5], [65, 77.0], [66, 83.0], [67, 79.0], [68, 80.9], [69, 81.5], [70, 80.0]]
    cr = edge + [[40 + 7 * i, 148 + 4 * (i % 40)] for i in range(35)]
    inside = [0, 2, 7, 8, 9, 10]          # 78.0, 82.0 and the interior; below(78), above(82), 82.5 (bin 82 of the binned kernel), 77, 83 are absent
    return _row_case("row_band_edges", W, H, cl, cr, "left y 80.0 / 80.9 (both int() 80: band [78, 82]); right y 78, below 78, 82, above 82, 82.5",
                     claims={"members": {0: inside, 1: inside}, "min_ties": 0})


ROW_TOTALS = [0, 1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 3]
# the totals of consecutive left features: every four make one wavefront of the binned kernel.  (65, 3, 0, 64): all four through the long-window path
ROW_TOTAL_GROUPS = [(64, 0, 1, 17), (65, 3, 0, 64), (15, 16, 32, 33), (48, 49, 63, 1), (17, 65, 33, 0), (16, 48, 3, 15), (63, 32, 49, 64)]


def row_window_totals():
    W, H = 320, 400
    centre = {t: 40 + 11 * k for k, t in enumerate(ROW_TOTALS)}        # bands of 5 rows, 6 rows between them
    cr = []
    for t in ROW_TOTALS:
        b = _band(centre[t], t)
        if t >= 15:
            b[-1] = list(b[0])                                         # a duplicate corner: the same descriptor at two indices
        cr += b
    order = [t for g in ROW_TOTAL_GROUPS for t in g]
    cl = [[40 + 5 * i + (0.5 if i % 3 == 1 else 0.0), centre[t] + (0.75 if i % 2 else 0.0)] for i, t in enumerate(order)]
    return _row_case("row_window_totals", W, H, cl, cr, "bands of 0, 1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65 right features, mixed within the groups of four",
                     claims={"counts": order, "min_ties": 60})


ROW_CAPACITY = [127, 128, 129, 191, 192, 193, 300, 5]


def row_capacity():
    W, H = 320, 400
    centre = {t: 40 + 12 * k for k, t in enumerate(ROW_CAPACITY)}
    cr = []
    for t in ROW_CAPACITY:
        b = _band(centre[t], t, step=4)
        b[-1] = list(b[1])
        cr += b
    order = [127, 128, 129, 191, 192, 193, 300, 5, 128, 5, 300, 129, 192, 127, 193, 191]
    cl = [[40 + 9 * i, centre[t] + (0.5 if i % 2 else 0.0)] for i, t in enumerate(order)]
    return _row_case("row_capacity", W, H, cl, cr, "bands of 127, 128 (KC), 129, 191, 192 (the long window's key segment), 193 and 300 right features",
                     claims={"counts": order, "min_ties": 200})


def row_train_count(n_right, n_left=48):
    W, H = 320, 400
    rng = np.random.default_rng([11, n_right, n_left])
    cl, cr = scatter(rng, n_left, W, H), scatter(rng, n_right, W, H)
    if n_right:
        cr[0] = cl[0]                                                  # at least one list is not empty
    return _row_case(f"row_train_{n_right}_{n_left}", W, H, cl, cr, f"{n_right} right features, {n_left} left",
                     claims={"n_right": n_right, "n_left": n_left, "min_ties": 0 if n_right < 1000 else 50},
                     expect={"stood_down_row": 1 if n_right > LS_NMAX else 0})


def row_query_count(n_left, wgs):
    W, H = 320, 400
    rng = np.random.default_rng([13, n_left])
    cl, cr = scatter(rng, n_left, W, H), scatter(rng, 600, W, H)
    cr[0] = cl[0]
    return _row_case(f"row_queries_{n_left}_wgs{wgs}", W, H, cl, cr, f"{n_left} left features (chunks of 256, parts rounded up to 64) over {wgs} workgroups",
                     claims={"n_right": 600, "n_left": n_left, "min_ties": 0}, env={"LVT_AMD_LISTS_WGS": f"{wgs},1"})


def row_bins(H):
    W = 96
    rng = np.random.default_rng([17, H])
    cl, cr = scatter(rng, 64, W, H), scatter(rng, 400, W, H)
    cl[:4] = [[40, H - 29], [41, H - 30], [42, BORDER], [43, H - 31]]
    cr[:6] = [[50, H - 29], [51, H - 29.4], [52, H - 31], [53, BORDER], [54, BORDER + 2], [55, H - 28.6]]
    return _row_case(f"row_bins_{H}", W, H, cl, cr, f"{H + 1} row bins", claims={"n_right": 400, "n_left": 64, "min_ties": 0},
                     expect={"stood_down_row": 1 if H + 1 > LS_BINS else 0})


def row_third_builder():
    c = row_window_totals()
    c["name"], c["env"] = "row_third_builder", {"LVT_AMD_TEST_ROW_FALLBACK": "1"}
    c["plants"] += "; k_triangulate builds the lists itself while the early stream's builder writes the same words"
    c["expect"]["row_fallback"] = 1
    return c


ROW_CASES = {"row_band_edges": row_band_edges, "row_window_totals": row_window_totals, "row_capacity": row_capacity, "row_third_builder": row_third_builder}
for _n in (0, 1, 63, 64, 65, 1535, 1536, 1537):
    ROW_CASES[f"row_train_{_n}"] = functools.partial(row_train_count, _n)
ROW_CASES["row_train_4096"] = functools.partial(row_train_count, 4096, 4096)    # NF_MAX on both sides: only the wavefront-per-query builder takes it
for _n in (1, 63, 64, 65, 255, 256, 257, 513):
    for _w in (1, 2, 4):
        ROW_CASES[f"row_queries_{_n}_wgs{_w}"] = functools.partial(row_query_count, _n, _w)
for _h in (1099, 1100):
    ROW_CASES[f"row_bins_{_h}"] = functools.partial(row_bins, _h)


def check_row_claims(case, xy_l, xy_r, ref):
    """what a row case claims, on the features a tracker (the oracle, or the device) made of its corners and the reference lists over them"""
    W, H = case["W"], case["H"]
    _, _, cl, cr = case["frames"][0]
    assert np.array_equal(np.asarray(xy_l, f32), survivors(cl, W, H)) and np.array_equal(np.asarray(xy_r, f32), survivors(cr, W, H)), "the features are not the planted corners"
    c = case["claims"]
    if "n_left" in c:
        assert (len(xy_l), len(xy_r)) == (c["n_left"], c["n_right"])
    if "counts" in c:
        assert ref["counts"].tolist() == c["counts"]
    for q, members in c.get("members", {}).items():
        assert np.flatnonzero(ref["mask"][q]).tolist() == sorted(members), (q, np.flatnonzero(ref["mask"][q]))
    assert LU.equal_distance_neighbours(ref["full"]) >= c["min_ties"], LU.equal_distance_neighbours(ref["full"])
    if len(xy_l) and len(xy_r):
        yl = np.asarray(xy_l, f32)[:, 1]
        assert yl.astype(int).min() - 2 > 0 and yl.astype(int).max() + 2 < H            # (the clips at 0 and H are out of reach, see the module text)


# ================================================================================================================================================================
# map cases
# ================================================================================================================================================================
def map_params(W, H, radius, staged_threshold=0, min_matches=10):
    prm = lvt_amd.kitti_params(width=W, height=H, fx=200.0, fy=200.0, cx=W / 2.0, cy=H / 2.0, baseline=0.4)      # disparity 8 px at z = 10 m
    prm.tracking_radius, prm.triangulation_policy, prm.staged_threshold, prm.untracked_threshold = radius, 2, staged_threshold, 1000
    prm.min_num_matches_for_tracking = min_matches
    return prm


def on_circle(radius):
    """integer offsets exactly on the radius: dx * dx + dy * dy == r * r (both axes, and every lattice point of the first quadrant)"""
    return [(a, b) for a in range(radius + 1) for b in range(radius + 1) if a * a + b * b == radius * radius]


def _stereo(left_corners):
    cl = np.asarray(left_corners, np.float64).reshape(-1, 2)
    return cl, cl - [DISP, 0]


def _map_case(name, W, H, radius, P0, P1, planted, plants, claims, expect=None, env=None, staged_threshold=0, frame2=None, min_matches=10):
    left, right = noise_pair(W, H)
    P0, P1 = np.asarray(P0, np.float64).reshape(-1, 2), np.asarray(P1, np.float64).reshape(-1, 2)
    f2 = np.vstack([P0, P1, np.asarray(planted, np.float64).reshape(-1, 2)]) if frame2 is None else np.asarray(frame2, np.float64).reshape(-1, 2)
    frames = [(left, right) + _stereo(P0), (left, right) + _stereo(np.vstack([P0, P1])), (left, right) + _stereo(f2)]
    return dict(name=name, kind="map", W=W, H=H, radius=radius, prm=map_params(W, H, radius, staged_threshold, min_matches), frames=frames, P0=P0, P1=P1, plants=plants,
                claims=claims, expect=dict({"stood_down_map": 0, "pass2": 0}, **(expect or {})), env=dict({"LVT_AMD_ORDERING": "polling"}, **(env or {})))


def _lattice(W, H):
    """44 points: a lattice with room for a radius of 51 px towards +x / +y ... and four whose 5 x 5 cell window (radius 30) loses a column or a row at the grid's edge:
    hash column / row 1 and the last but one"""
    pts = [[x, y] for y in (40, 60, 80, 106) for x in range(44, 44 + 10 * 28, 28)]
    return pts + [[40, 44], [W - 40, H - 40], [40, H - 44], [W - 40, 44]]


def map_radius(radius, W=400, H=200, name=None, extra0=0, env=None, expect=None, pass2=False, min_matches=10):
    """the radius plants: every offset exactly on r^2 (absent), one row inside (present), around 40 lattice points; features on cell edges (x = 25 k and the
    fp32 number below it, the same in y).  extra0: further P0 points (the early count)"""
    rng = np.random.default_rng([19, radius, W, H, extra0])
    lat = np.array(_lattice(W, H), np.float64)
    offs = on_circle(radius)
    planted = [[x + a, y + b] for x, y in lat[:40] for a, b in offs] + [[x + a, y + b - 1] for x, y in lat[:40] for a, b in offs if b > 0 and a > 0]
    planted += [[25.0 * k, 50 + 3 * k] for k in range(2, 15)] + [[below(25.0 * k), 52 + 3 * k] for k in range(2, 15)]
    planted += [[60 + 7 * k, 25.0 * k] for k in range(2, 7)] + [[64 + 7 * k, below(25.0 * k)] for k in range(2, 7)]
    free = scatter(rng, extra0 + 30, W, H, x0=50, y0=132 if H <= 200 else 140, x1=W - 50, y1=H - 30)
    P0 = np.vstack([lat, free[:extra0]])
    P1 = free[extra0:]
    frame2 = None
    if pass2:   # (offsets on the DOUBLED radius too: those inside the cell window must be absent from the second pass's lists)
        planted += [[x + a, y + b] for x, y in lat[:40] for a, b in on_circle(2 * radius)]
    if pass2:   # fewer than 50 map points find their corner again: pass 1 ends below N_MATCHES_TH and the doubled radius runs over the same cell window
        frame2 = np.vstack([P0[:30], np.asarray(planted, np.float64)])
    name = name or f"map_radius_{radius}"
    csr = LU.cell_search_radius(radius)
    return _map_case(name, W, H, radius, P0, P1, planted, f"radius {radius} (cell search radius {csr}): offsets {offs} exactly on r^2, cell-edge features, clipped windows",
                     claims={"min_exact_r2": 8, "n0": len(P0), "n1": len(P1), "min_ties": 20, "clipped": radius == 30, "pass2": pass2},
                     expect=dict({"stood_down_map": 1 if csr > 2 else 0, "pass2": 1 if pass2 else 0}, **(expect or {})), env=env, frame2=frame2, min_matches=min_matches)


def _nearest(n):
    """the n integer offsets nearest to (0, 0), itself first: all within 12 px"""
    o = [(a, b) for a in range(-12, 13) for b in range(-12, 13)]
    o.sort(key=lambda p: (p[0] * p[0] + p[1] * p[1], p))
    return o[:n]


def map_totals(staged=False):
    """blocks of corners at 1-px spacing: exactly 63, 64 and 65 features in a point's window cells (40 of them inside the radius: total != inside), exactly 127, 128,
    129 and 200 (> 192) features inside a point's radius.  The points' 3 x 3 cell windows are disjoint: hash rows 0-2 (y < 75), 3-4 (75 <= y < 125; row 5 stays
    empty) and 6 (150 <= y), hash columns 1-3, 6-8, 11-13.  staged: the same blocks around STAGED points (a map of 250 points and more stages what frame 1
    triangulates), 128 and 129 among them"""
    W, H, radius = 400, 200, 25
    rng = np.random.default_rng([23, int(staged)])
    targets = [((62, 40), 63, 40), ((187, 40), 64, 40), ((312, 40), 65, 40), ((62, 100), None, 127), ((187, 100), None, 128), ((312, 100), None, 129), ((62, 160), None, 200)]
    pts, planted, want = [], [], []
    for (x, y), total, inside in targets:
        pts.append([x, y])
        near = [(a, b) for a, b in _nearest(600) if BORDER <= y + b < H - BORDER and (y != 160 or y + b >= 150)][:inside]
        planted += [[x + a, y + b] for a, b in near[1:]]                       # (the point's own corner is one of them)
        if total is not None:
            planted += [[x + 27 + (k % 10), y + 8 + k // 10] for k in range(total - inside)]      # in the window's cells, outside the radius
        want.append((x, y, total, inside))
    fill = scatter(rng, 300, W, H, x0=150, y0=150, x1=W - 30, y1=H - 30)
    if staged:   # 260 map points first; the planted points come with frame 1 and are staged
        P0, P1 = fill[:260], np.vstack([np.array(pts, np.float64), fill[260:290]])
    else:
        P0, P1 = np.vstack([np.array(pts, np.float64), fill[:20]]), fill[20:50]
    return _map_case("staged_totals" if staged else "map_totals", W, H, radius, P0, P1, planted,
                     "window totals 63 / 64 / 65 (40 inside the radius), 127 / 128 / 129 / 200 inside the radius" + (" around staged points" if staged else ""),
                     claims={"totals": want, "n0": len(P0), "n1": len(P1), "min_ties": 100, "staged": staged}, staged_threshold=2 if staged else 0)


MAP_CASES = {f"map_radius_{r}": functools.partial(map_radius, r) for r in (25, 30, 50, 51)}
MAP_CASES["map_totals"] = map_totals
MAP_CASES["staged_totals"] = functools.partial(map_totals, True)
MAP_CASES["map_pass2"] = functools.partial(map_radius, 25, name="map_pass2", pass2=True)
MAP_CASES["map_cells_1100"] = functools.partial(map_radius, 25, 1100, 625, "map_cells_1100")
MAP_CASES["map_cells_1144"] = functools.partial(map_radius, 25, 1100, 650, "map_cells_1144", expect={"stood_down_map": 1})
for _e in (255, 256, 257):
    for _w in (1, 2, 4):
        MAP_CASES[f"map_early_{_e}_wgs{_w}"] = functools.partial(map_radius, 25, name=f"map_early_{_e}_wgs{_w}", extra0=_e - 44, env={"LVT_AMD_LISTS_WGS": f"2,{_w}"})


def nominal_projection(prm, xyz):
    """a map point seen from the identity pose, as the fp32 pair the tracker files: where the static camera's projections lie"""
    X = np.asarray(xyz, np.float64).reshape(-1, 3)
    return np.column_stack([prm.fx * X[:, 0] / X[:, 2] + prm.cx, prm.fy * X[:, 1] / X[:, 2] + prm.cy]).astype(f32)


def check_map_claims(case, proj, vis, xy, ref, n_early=None, which="map"):
    """what a map case claims, on the projections (the device's own; in the CPU tier the nominal ones of the oracle's map), frame 2's features and the
    reference lists over them"""
    c, W, H, radius = case["claims"], case["W"], case["H"], case["radius"]
    proj, xy = np.asarray(proj, f32).reshape(-1, 2), np.asarray(xy, f32).reshape(-1, 2)
    assert np.array_equal(xy, survivors(case["frames"][2][2], W, H)), "frame 2's features are not the planted corners"
    assert np.asarray(vis).astype(bool).all()
    staged = c.get("staged", False)
    if which == "map":
        assert len(proj) == c["n0"] + (0 if staged else c["n1"]), (len(proj), c["n0"], c["n1"])
        if n_early is not None:
            assert 0 < n_early < len(proj) or staged, n_early
            assert n_early == c["n0"] or staged, (n_early, c["n0"])
        nominal = case["P0"] if staged else np.vstack([case["P0"], case["P1"]])
    else:
        assert len(proj) == c["n1"]
        nominal = case["P1"]
    d = np.abs(proj[:, None, :] - nominal[None, :, :].astype(f32)).max(axis=2)        # every projection lies on a planted position (the order is the tracker's)
    assert (d.min(axis=1) < 1e-3).all() and len(set(d.argmin(axis=1).tolist())) == len(proj), d.min(axis=1).max()
    assert LU.equal_distance_neighbours(ref["full"]) >= c["min_ties"], LU.equal_distance_neighbours(ref["full"])
    if "min_exact_r2" in c and which == "map":
        r = radius * (2 if c["pass2"] else 1)
        d2 = LU.track_d2(proj, xy)
        exact = int(((d2 == f32(radius * radius)) & ref["cells"]).sum())
        assert exact >= c["min_exact_r2"], exact                                        # pairs exactly on r^2 in fp32 (absent from a pass-1 list)
        if not c["pass2"]:
            assert not (ref["mask"] & (d2 == f32(r * r))).any()
        else:
            assert int((ref["cells"] & (d2 == f32(r * r))).sum()) >= 1                  # (14, 48), (30, 40) ... on the doubled radius, in the window
            assert int((~ref["cells"] & (d2 < f32(r * r)) & (d2 >= f32(radius * radius))).sum()) >= 8   # inside the doubled radius, outside the cell window: absent
    if c.get("clipped"):
        w = LU.track_window(proj, radius, W, H)
        ccx, ccy = LU.hash_grid(W, H)
        assert ((w[:, 1] - w[:, 0] == 4) & (w[:, 0] == 0)).any() and ((w[:, 1] - w[:, 0] == 4) & (w[:, 1] == ccx)).any()
        assert ((w[:, 3] - w[:, 2] == 4) & (w[:, 2] == 0)).any() and ((w[:, 3] - w[:, 2] == 4) & (w[:, 3] == ccy)).any()
    if "totals" in c and (which == "staged") == staged:
        for x, y, total, inside in c["totals"]:
            q = int(np.abs(proj - np.array([x, y], f32)).max(axis=1).argmin())
            assert int(ref["counts"][q]) == inside, (x, y, int(ref["counts"][q]), inside)
            if total is not None:
                assert int(ref["cells"][q].sum()) == total, (x, y, int(ref["cells"][q].sum()), total)
