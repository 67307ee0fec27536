"""The inputs of the edge-case tests of relocalisation's correspondence stage (include/lvt_amd_ext.h, RELOCALISATION, stage 2; k_reloc_corr, k_reloc_points
and k_reloc_list behind k_reloc_match), in one place: tests/test_gpu_reloc_correspond.py drives lvt_amd_reloc_correspond with them, the CPU tier
(tests/test_reloc.py) asserts with tests/reloc_util.py alone that each case still has the property it is named for.  Nothing here needs a GPU.

A case is a dict: prm, sensor, xy_l, desc_l, right = (xy_r, desc_r) or None, depth or None, map_xyz, map_desc, other = (xyz, desc) of the map copy that is
not live or None, map_copy, lost_frame, min_disparity, `plants` (a sentence) and `check(case, ref)`, which raises AssertionError when the case has lost its
property.  restate(case) is the answer of the definition.

Descriptors are random bytes; a match is planted by copying a descriptor and flipping a chosen number of bits.  Two unrelated random 256-bit descriptors are
about 128 bits apart (the nearest of some thousands: 85 or more), so a feature is accepted only where it was planted.  The kernels' constants that the shapes
lean on: a workgroup of 1024 threads owns feature i in pass i / 1024 (k_reloc_corr) and correspondence c in block c / 1024 (k_reloc_list); a wavefront of 64
lanes walks the right features, lane j % 64 (k_reloc_points)."""
import dataclasses
import functools

import numpy as np

import lvt_amd
import reloc_util as RU

W, H = 1241, 376


def params(track=0.75, tri=0.75, desc_th=30.0, kind="kitti"):
    """0.75 is exact in fp32 (the defaults 0.8, 0.7 and 0.6 are not): a ratio of exactly 0.75 is an equality case"""
    base = {"kitti": lvt_amd.kitti_params, "tum": lvt_amd.tum_params}[kind]()
    return dataclasses.replace(base, tracking_ratio_test_threshold=track, triangulation_ratio_test_threshold=tri, descriptor_matching_threshold=desc_th)


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def near(rng, desc, k):
    """a copy of desc with k distinct bits flipped: Hamming distance exactly k"""
    d = np.array(desc, np.uint8).copy()
    for b in rng.choice(256, int(k), replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _case(**kw):
    c = dict(sensor=1, right=None, depth=None, other=None, map_copy=0, lost_frame=0, min_disparity=1.0, check=lambda case, ref: None)
    c.update(kw)
    c["xy_l"] = np.ascontiguousarray(c["xy_l"], np.float32).reshape(-1, 2)
    c["desc_l"] = np.ascontiguousarray(c["desc_l"], np.uint8).reshape(-1, 32)
    c["map_xyz"] = np.ascontiguousarray(c["map_xyz"], np.float64).reshape(-1, 3)
    c["map_desc"] = np.ascontiguousarray(c["map_desc"], np.uint8).reshape(-1, 32)
    if c["right"] is not None:
        c["right"] = (np.ascontiguousarray(c["right"][0], np.float32).reshape(-1, 2), np.ascontiguousarray(c["right"][1], np.uint8).reshape(-1, 32))
    return c


def restate(case):
    """stages 1 and 2 by tests/reloc_util.py: the records, the correspondences and every output of lvt_amd_reloc_correspond, trimmed to the counts"""
    prm, M = case["prm"], len(case["map_xyz"])
    rec = RU.global_match(case["desc_l"], case["map_desc"])
    feat, mp, n_matched = RU.correspondences(rec, M, prm.tracking_ratio_test_threshold, prm.descriptor_matching_threshold)
    if case["sensor"] == 2:
        pc, has = RU.camera_points_rgbd(feat, case["xy_l"], case["depth"], prm)
    else:
        xy_r, desc_r = case["right"] if case["right"] is not None else (np.zeros((0, 2), np.float32), np.zeros((0, 32), np.uint8))
        pc, has = RU.camera_points_stereo(feat, case["xy_l"], case["desc_l"], xy_r, desc_r, prm, case["min_disparity"], prm.img_height)
    with_pc = np.flatnonzero(has)
    return dict(records=rec, feat=feat, map_idx=mp, X=case["map_xyz"][mp].reshape(-1, 3), uv=case["xy_l"][feat].reshape(-1, 2), pc=pc, has_pc=has, with_pc=with_pc,
                n_features=len(case["xy_l"]), n_map=M, n_matched=n_matched, n_corr=len(feat), n_with_point=len(with_pc), status=1 if len(with_pc) < 3 else -1)


def partner_of(case, ref, i):
    """the right feature the definition pairs left feature i with (None: no point, or i is no correspondence): read back from Z = fx b / (x_l - x_r)"""
    c = np.flatnonzero(ref["feat"] == i)
    if len(c) == 0 or not ref["has_pc"][c[0]]:
        return None
    prm = case["prm"]
    xl = float(case["xy_l"][i, 0])
    fxb = float(np.float32(prm.fx)) * float(np.float32(prm.baseline))
    j = [k for k, xr in enumerate(case["right"][0][:, 0]) if xl != float(xr) and fxb / (xl - float(xr)) == ref["pc"][c[0], 2]]
    assert len(j) >= 1, i
    return j


# ---- the generic scene: A (sizes), F (RGB-D), G (map copy, LOST counts) --------------------------------------------------------------------------------
def scene(N, M, seed, n_right=None, sensor=1, prm=None, decoys=False, map_copy=0, lost_frame=0, plants=""):
    """N left features at fractional coordinates, about three in four planted (0 ... 20 bits off) on distinct map points -- where the map has fewer points
    than that, on point i mod M, so the points are contested.  Stereo: 85 in 100 planted features have a partner in the right image (the same row, 5 ... 60
    px to the left, 0 ... 8 bits off); the right features are shuffled, and topped up with random ones to n_right.  RGB-D: a depth of 0.5 ... 8 m each."""
    rng = np.random.default_rng(seed)
    prm = prm or (params(0.8, 0.6) if sensor == 1 else params(0.7, 0.6, kind="tum"))
    Hh, Ww = prm.img_height, prm.img_width
    map_desc, map_xyz = rand_desc(rng, M), rng.normal(0, 10, (M, 3))
    xy = np.column_stack([rng.uniform(70, Ww - 1, N), rng.uniform(0, Hh - 0.01, N)]).astype(np.float32)
    desc = rand_desc(rng, N)
    planted = np.flatnonzero(rng.random(N) < 0.75)
    if M > 0:
        target = rng.permutation(M)[:len(planted)] if len(planted) <= M else planted % M
        for i, m in zip(planted, target):
            desc[i] = near(rng, map_desc[m], rng.integers(0, 61 if M == 1 else 21))
    kw = {}
    if sensor == 2:
        kw["depth"] = rng.uniform(0.5, 8.0, N).astype(np.float32)
    else:
        with_partner = planted[rng.random(len(planted)) < 0.85]
        if n_right is not None:
            with_partner = with_partner[:n_right]
        n_r = len(with_partner) if n_right is None else n_right
        xy_r = np.column_stack([rng.uniform(0, Ww - 1, n_r), rng.uniform(0, Hh - 0.01, n_r)]).astype(np.float32)
        desc_r = rand_desc(rng, n_r)
        slot = rng.permutation(n_r)[:len(with_partner)]
        for i, j in zip(with_partner, slot):
            xy_r[j] = (xy[i, 0] - np.float32(rng.uniform(5, 60)), xy[i, 1])
            desc_r[j] = near(rng, desc[i], rng.integers(0, 9))
        kw["right"] = (xy_r, desc_r)
    if decoys:      # the copy that is NOT live: every feature's own descriptor (distance 0) at some index, other positions everywhere
        od, ox = rand_desc(rng, M), map_xyz[::-1] + 1000.0
        where = rng.permutation(M)[:min(N, M)]
        od[where] = desc[:len(where)]
        kw["other"] = (ox, od)
    return _case(prm=prm, sensor=sensor, xy_l=xy, desc_l=desc, map_xyz=map_xyz, map_desc=map_desc, map_copy=map_copy, lost_frame=lost_frame, plants=plants, **kw)


def _check_sizes(case, ref):
    N, M = len(case["xy_l"]), len(case["map_xyz"])
    if M == 0:
        assert ref["n_matched"] == 0 and ref["n_corr"] == 0 and ref["status"] == 1
    if M == 1 and N > 100:      # the one-candidate rule, both ways, and every accepted feature claims the one point
        d1 = ref["records"][:, 1]
        assert (d1 <= 30).sum() > 50 and (d1 > 30).sum() > 50 and ref["n_matched"] == int((d1 <= 30).sum()) and ref["n_corr"] == 1
    if 1 < M < N // 2:
        assert ref["n_corr"] == M and ref["n_matched"] > M             # every point contested
    if N >= 2049 and M >= 3000:
        assert ref["n_corr"] > 1024
    if N == 4096 and M >= 3000:
        assert ref["n_corr"] > 2048 and ref["n_with_point"] > 2048
    if N >= 2049 and M >= 3000 and case["sensor"] == 1:                 # the second compaction is not the identity, either side of block 1024
        assert not ref["has_pc"][:1024].all() and not ref["has_pc"][1024:].all() and ref["has_pc"][:1024].any() and ref["has_pc"][1024:].any()
    if N >= 1023 and M >= 3000:
        assert 0.6 * N < ref["n_corr"] <= ref["n_matched"] < 0.9 * N


def sizes_cases():
    out = {}
    for N in (0, 1, 1023, 1024, 1025, 2049, 4096):
        out[f"A-N{N}-M3300"] = lambda N=N: dict(scene(N, 3300, 10 + N, plants=f"{N} left features against 3300 map points, three in four planted"), check=_check_sizes)
    for M in (0, 1, 2, 33):
        out[f"A-N1025-M{M}"] = lambda M=M: dict(scene(1025, M, 20 + M, plants=f"1025 features against a map of {M}: cnt = min(M, 2), every point contested"),
                                                check=_check_sizes)
    out["A-N4096-M32768"] = lambda: dict(scene(4096, 32768, 31, n_right=4096, plants="capacity: 4096 left, 4096 right, 32768 map points"), check=_check_sizes)
    return out


# ---- B: the accept rule ------------------------------------------------------------------------------------------------------------------------------------
PAIRS_075 = [((0, 0), False), ((0, 5), True), ((3, 4), False), ((96, 128), False), ((95, 128), True), ((97, 128), False)]
PASS_SPOTS = lambda p: [1024 * k + 5 + 67 * p for k in range(4)]     # pair p of a table: once in each of the four passes, at i, i + 1024, i + 2048, i + 3072


def pairs_at_default(th=0.8):
    """the integer pairs (d1, d2), d2 <= 256, whose fp32 quotient is the nearest below fp32(th) (accepted), equal to it (the one with the largest d2) and the
    nearest above (both rejected): from the number format alone.  For 0.8: (203, 254), (204, 255), (205, 256)."""
    t = np.float32(th)
    q = {(a, b): np.float32(a) / np.float32(b) for b in range(1, 257) for a in range(0, b + 1)}
    below = max((k for k in q if q[k] < t), key=lambda k: (q[k], k[1]))
    above = min((k for k in q if q[k] > t), key=lambda k: (q[k], -k[1]))
    equal = sorted((k for k in q if q[k] == t), key=lambda k: -k[1])[:1]
    return [(below, True)] + [(k, False) for k in equal] + [(above, False)]


def accept_case(pairs, track, seed, plants):
    """small distances against a map of some hundred random points (85 bits or more from everything): for every (d1, d2) of `pairs` and every pass a map
    point d1 bits and another d2 bits from the feature"""
    rng = np.random.default_rng(seed)
    N, M0 = 4096, 300
    desc = rand_desc(rng, N)
    extra, spots = [], {}
    for p, ((d1, d2), ok) in enumerate(pairs):
        assert d2 < 60
        for i in PASS_SPOTS(p):
            spots[i] = (d1, d2, ok, M0 + len(extra))
            extra += [near(rng, desc[i], d1), near(rng, desc[i], d2)]
    map_desc = np.vstack([rand_desc(rng, M0), np.array(extra, np.uint8)])
    M = len(map_desc)
    xy = np.column_stack([rng.uniform(70, W - 1, N), rng.uniform(0, H - 0.01, N)])

    def check(case, ref):
        got = set(ref["feat"].tolist())
        for i, (d1, d2, ok, m) in spots.items():
            assert ref["records"][i].tolist() == [m, d1, m + 1, d2], (i, ref["records"][i])
            assert RU.accept_match(2, d1, d2, track, 30.0) == ok and (i in got) == ok, (i, d1, d2)
        assert sorted(i // 1024 for i in spots) == sorted(list(range(4)) * len(pairs)) and {ok for _, ok in pairs} == {True, False}
    return _case(prm=params(track, 0.6), xy_l=xy, desc_l=desc, map_xyz=rng.normal(0, 10, (M, 3)), map_desc=map_desc, plants=plants, check=check)


def two_point_case(pairs, track, seed, plants):
    """large distances: random descriptors sit about 128 bits from everything, so a second best of 128 or more needs a map of TWO points, A and B = A with w
    bits flipped.  A feature d1 from A and d2 from B is A with o = (d1 + w - d2) / 2 of those w bits and d1 - o of the others flipped; w is the first width
    that gives every pair of the table a whole o.  Every accepted feature claims A: the decision shows in n_matched and in who keeps the point."""
    rng = np.random.default_rng(seed)
    N = 4096
    fits = lambda w, d1, d2: (d1 + w - d2) % 2 == 0 and 0 <= (d1 + w - d2) // 2 <= min(w, d1) and d1 - (d1 + w - d2) // 2 <= 256 - w
    w = next(w for w in range(1, 256) if all(fits(w, *pr) for pr, _ in pairs))
    A = rand_desc(rng, 1)[0]
    bits = rng.permutation(256)
    inside, outside = bits[:w], bits[w:]
    flip = lambda d, which: [d.__setitem__(b >> 3, d[b >> 3] ^ np.uint8(1 << (b & 7))) for b in which]
    B = A.copy(); flip(B, inside)
    desc = rand_desc(rng, N)
    spots = {}
    for p, ((d1, d2), ok) in enumerate(pairs):
        o = (d1 + w - d2) // 2
        for i in PASS_SPOTS(p):
            q = A.copy(); flip(q, rng.permutation(inside)[:o]); flip(q, rng.permutation(outside)[:d1 - o])
            desc[i], spots[i] = q, (d1, d2, ok)
    xy = np.column_stack([rng.uniform(70, W - 1, N), rng.uniform(0, H - 0.01, N)])

    def check(case, ref):
        for i, (d1, d2, ok) in spots.items():
            assert ref["records"][i].tolist() == [0, d1, 1, d2], (i, ref["records"][i])
            assert RU.accept_match(2, d1, d2, track, 30.0) == ok, (d1, d2)
        r = ref["records"]
        others = np.delete(np.arange(N), list(spots))
        acc = sum(RU.accept_match(2, int(r[i, 1]), int(r[i, 3]), track, 30.0) for i in others)
        assert ref["n_matched"] == acc + sum(ok for _, _, ok in spots.values())
        assert sorted(i // 1024 for i in spots) == sorted(list(range(4)) * len(pairs))
    return _case(prm=params(track, 0.6), xy_l=xy, desc_l=desc, map_xyz=rng.normal(0, 10, (2, 3)), map_desc=np.stack([A, B]), plants=plants, check=check)


def one_point_case():
    """a map of ONE point: d1 == descriptor_matching_threshold is accepted, one above is not; in every pass"""
    rng = np.random.default_rng(41)
    N = 4096
    desc, map_desc = rand_desc(rng, N), rand_desc(rng, 1)
    at, above = [1024 * k + 300 + k for k in range(4)], [1024 * k + 301 + k for k in range(4)]
    for i in at:
        desc[i] = near(rng, map_desc[0], 30)
    for i in above:
        desc[i] = near(rng, map_desc[0], 31)
    xy = np.column_stack([rng.uniform(70, W - 1, N), rng.uniform(0, H - 0.01, N)])

    def check(case, ref):
        d1 = ref["records"][:, 1]
        assert (d1[at] == 30).all() and (d1[above] == 31).all() and (np.delete(d1, at + above) > 31).all()
        assert ref["n_matched"] == 4 and ref["feat"].tolist() == [at[0]]
    return _case(prm=params(0.75, 0.6, 30.0), xy_l=xy, desc_l=desc, map_xyz=rng.normal(0, 10, (1, 3)), map_desc=map_desc, check=check,
                 plants="one map point: d1 = 30 = descriptor_matching_threshold accepted, 31 rejected, in each pass; the lowest accepted feature keeps the point")


# ---- C: the mutual filter ------------------------------------------------------------------------------------------------------------------------------------
def claim_case(which):
    rng = np.random.default_rng(50 + which)
    N = 4096
    desc = rand_desc(rng, N)
    xy = np.column_stack([rng.uniform(70, W - 1, N), rng.uniform(0, H - 0.01, N)])
    if which in (1, 2):
        # 64 features, 16 in each pass, 61 apart (15 of a pass's 16 wavefronts): all claim map point 17.  (i) equal d1; (ii) a smaller d1 at the highest
        M = 300
        map_desc = rand_desc(rng, M)
        idx = [1024 * k + 3 + 61 * j for k in range(4) for j in range(16)]
        for i in idx:
            desc[i] = near(rng, map_desc[17], 4 if (which == 2 and i == idx[-1]) else 9)
        winner = idx[0] if which == 1 else idx[-1]

        def check(case, ref):
            r = ref["records"][idx]
            assert (r[:, 0] == 17).all() and (r[:-1, 1] == 9).all() and r[-1, 1] == (9 if which == 1 else 4)
            assert len({i // 1024 for i in idx}) == 4 and len({(i % 1024) // 64 for i in idx}) > 8
            assert ref["n_matched"] >= 64 and [i for i in ref["feat"].tolist() if i in idx] == [winner] and ref["map_idx"][ref["feat"] == winner] == 17
        plants = ("64 features over four passes claim one point with equal d1: the lowest index keeps it" if which == 1 else
                  "64 features over four passes claim one point, the highest index with a strictly smaller d1: it keeps it")
    elif which == 3:
        M = 50
        map_desc = rand_desc(rng, M)
        for i in range(N):
            desc[i] = near(rng, map_desc[13], rng.integers(2, 21))

        def check(case, ref):
            d1 = ref["records"][:, 1]
            assert ref["n_matched"] == 4096 and ref["n_corr"] == 1 and ref["feat"][0] == int(np.flatnonzero(d1 == d1.min())[0]) and (d1 == d1.min()).sum() > 1
        plants = "all 4096 features claim one map point: n_matched 4096, n_corr 1, the lowest index among the smallest d1"
    else:
        M = 2100
        map_desc = rand_desc(rng, M)
        target = rng.permutation(M)[:2048]
        for i in range(2048):
            desc[i], desc[i + 2048] = near(rng, map_desc[target[i]], rng.integers(0, 6)), near(rng, map_desc[target[i]], rng.integers(0, 6))

        def check(case, ref):
            d = ref["records"][:, 1]
            lo, hi, tie = (d[:2048] < d[2048:]).sum(), (d[:2048] > d[2048:]).sum(), (d[:2048] == d[2048:]).sum()
            assert min(lo, hi, tie) > 100 and ref["n_matched"] == 4096 and ref["n_corr"] == 2048
            keep = np.where(d[:2048] <= d[2048:], np.arange(2048), np.arange(2048) + 2048)
            assert ref["feat"].tolist() == sorted(keep.tolist())
        plants = "features i and i + 2048 (passes 0 / 2 and 1 / 3) claim the same point: 2048 contested points, won from either pass and by the tie rule"
    # a partner for every left feature, so a kept loser would show in Pc as well
    xy_r = np.column_stack([xy[:, 0] - rng.uniform(5, 60, N), xy[:, 1]])
    return _case(prm=params(0.75, 0.75), xy_l=xy, desc_l=desc, right=(xy_r, desc.copy()), map_xyz=rng.normal(0, 10, (M, 3)), map_desc=map_desc, plants=plants,
                 check=check)


# ---- D, E: the stereo partner ----------------------------------------------------------------------------------------------------------------------------------
def _stereo_subcases(subs, seed, n_right, plants, tri=0.75, filler_in_band=False):
    """subs: (name, (x_l, y_l), [(x_r, y_r, bits off the left descriptor, right index or None)], expected partner's position in that list or None).  Every left
    feature is planted on a map point of its own, so it is a correspondence; the fillers up to n_right lie right of every left feature (never a candidate)."""
    rng = np.random.default_rng(seed)
    n = len(subs)
    map_desc = rand_desc(rng, 200 + n)
    desc = np.array([near(rng, map_desc[200 + s], 2) for s in range(n)], np.uint8)
    xy = np.array([s[1] for s in subs], np.float64)
    xy_r = np.column_stack([rng.uniform(1235, 1240, n_right), rng.uniform(0, H, n_right)])
    desc_r = rand_desc(rng, n_right)
    free = [j for j in range(n_right - 1, -1, -1) if j not in {r[3] for s in subs for r in s[2] if r[3] is not None}]
    expect = {}
    for s, (name, _, rights, want) in enumerate(subs):
        for k, (xr, yr, bits, j) in enumerate(rights):
            j = free.pop() if j is None else j
            xy_r[j] = (xr, yr)
            desc_r[j] = near(rng, desc[s], bits)
            if want == k:
                expect[s] = j
        expect.setdefault(s, None)
    prm = params(0.75, tri)

    def check(case, ref):
        assert ref["feat"].tolist() == list(range(n))
        for s in range(n):
            got = partner_of(case, ref, s)
            assert (got is None and expect[s] is None) or (got is not None and expect[s] in got), (subs[s][0], got, expect[s])
    c = _case(prm=prm, xy_l=xy, desc_l=desc, right=(xy_r, desc_r), map_xyz=rng.normal(0, 10, (len(map_desc), 3)), map_desc=map_desc, plants=plants, check=check)
    c["expect"] = expect
    return c


def _in_band(yl, yr, rows=H):
    return np.float32(max(int(np.float32(yl)) - 2, 0)) <= np.float32(yr) <= np.float32(min(int(np.float32(yl)) + 2, rows))


def band_case():
    """the row band and the disparity predicate.  Every planted NON-candidate carries the left descriptor itself (0 bits off), the candidate 10 bits and a far
    second candidate 120: a predicate that admits the wrong one changes the partner, one that drops the right one leaves the far candidate alone (accepted
    alone, and one candidate at 120 > descriptor_matching_threshold is rejected), so either mistake shows."""
    one = np.float32(1.0)
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    far = lambda x, y: (x, y, 120, None)
    subs = [
        ("band lower edge: 7.99 out, 8.0 in", (600.5, 10.9), [(500.0, 7.99, 0, None), (510.0, 8.0, 10, None), far(520.0, 10.0)], 1),
        ("band upper edge: 12.0 in, 12.01 out", (600.5, 30.9), [(500.0, 32.01, 0, None), (510.0, 32.0, 10, None), far(520.0, 30.0)], 1),
        ("y_l < 2: the lower edge is 0", (600.5, 1.5), [(500.0, -0.5, 0, None), (510.0, 0.0, 10, None), far(520.0, 1.0), (530.0, 3.01, 0, None)], 1),
        ("y_l within two rows of img_height: the upper edge is img_height", (600.5, 374.6), [(500.0, 376.01, 0, None), (510.0, 376.0, 10, None), far(520.0, 373.0)], 1),
        ("y_l in the last row: the upper edge is img_height, not y + 2", (600.5, 375.2), [(500.0, 376.5, 0, None), (510.0, 376.0, 10, None), far(520.0, 373.5)], 1),
        ("disparity == min_disparity is a candidate", (600.5, 50.9), [(599.5, 50.0, 10, None), far(520.0, 51.0)], 0),
        ("disparity one ulp below min_disparity is none", (600.5, 70.9), [(up(599.5), 70.0, 0, None), (510.0, 70.0, 10, None), far(520.0, 71.0)], 1),
        ("disparity 0 is none", (600.5, 90.9), [(600.5, 90.0, 0, None), (510.0, 90.0, 10, None), far(520.0, 91.0)], 1),
        ("a negative disparity is none", (600.5, 110.9), [(605.5, 110.0, 0, None), (510.0, 110.0, 10, None), far(520.0, 111.0)], 1),
        # x_l - x_r = 1 - 2^-25 exactly: fp32 rounds it (to even) to 1.0, a candidate; compared in fp64 it would be none
        ("disparity rounds to min_disparity in fp32", (1.25, 130.9), [(0.25 + 2.0 ** -25, 130.0, 10, None), far(0.125, 131.0)], 0),
    ]
    c = _stereo_subcases(subs, 60, 64, "the band's two float edges, its clamps at 0 and img_height, and x_l - x_r at, one ulp below, zero, negative and rounding to min_disparity")
    inner = c["check"]

    def check(case, ref):
        inner(case, ref)
        xy_r = case["right"][0]
        cand = lambda s, j: bool(_in_band(case["xy_l"][s, 1], xy_r[j, 1]) and (case["xy_l"][s, 0] - xy_r[j, 0]) >= one)
        sides = []
        for s, (name, (xl, yl), rights, want) in enumerate(subs):           # both sides of each predicate, decided here from the text alone
            js = [int(np.flatnonzero((xy_r[:, 0] == np.float32(r[0])) & (xy_r[:, 1] == np.float32(r[1])))[0]) for r in rights]
            sides.append([cand(s, j) for j in js])
            assert cand(s, js[want]) and sides[-1].count(False) >= (0 if "==" in name or "rounds" in name else 1), name
        assert (np.float32(1.25) - np.float32(0.25 + 2.0 ** -25)) == one and (1.25 - float(np.float32(0.25 + 2.0 ** -25))) < 1.0
        assert (np.float32(600.5) - np.float32(up(599.5))) < one
        assert not _in_band(10.9, 7.99) and _in_band(10.9, 8.0) and _in_band(30.9, 32.0) and not _in_band(30.9, 32.01) and not _in_band(1.5, -0.5)
        assert _in_band(374.6, 376.0) and not _in_band(374.6, 376.01) and not _in_band(375.2, 376.5)
    c["check"] = check
    return c


def partner_case():
    """the partner choice among 4096 right features, at the exact triangulation ratio 0.75 and descriptor threshold 30.  j0 = a right index in lane 5; the
    named indices put best, second and third into the same lane one stride apart (j, j + 64) or into neighbouring lanes (j, j + 1)."""
    subs, y = [], 10.9

    def add(name, rights, want):
        nonlocal y
        subs.append((name, (700.5, y), [(600.0 - 3 * k, y - 0.9 + (k % 3), b, j) for k, (b, j) in enumerate(rights)], want))
        y += 7.0
    add("no candidate", [], None)
    add("one candidate at the descriptor threshold", [(30, None)], 0)
    add("one candidate one above the threshold", [(31, None)], None)
    add("two candidates, 95 / 128 < 0.75", [(95, None), (128, None)], 0)
    add("two candidates, 96 / 128 == 0.75", [(96, None), (128, None)], None)
    add("two candidates, 0 / 5", [(0, None), (5, None)], 0)
    add("two candidates, 0 / 0", [(0, None), (0, None)], None)
    j = 197                                                     # lane 5
    for name, order in (("best j, second j + 64 (the same lane), third j + 1", (0, 64, 1)), ("best j, second j + 1 (the next lane), third j + 64", (0, 1, 64)),
                        ("best j + 64, second j, third j + 1", (64, 0, 1)), ("best j + 1, second j + 64, third j", (1, 64, 0))):
        # a lost second best would let the third (200) decide: 96 / 200 passes, 96 / 128 does not -- and the other way round at 95
        add("rejected by its true second: " + name, [(96, j + order[0]), (128, j + order[1]), (200, j + order[2])], None)
        j += 200
        add("accepted by its true second: " + name, [(95, j + order[0]), (128, j + order[1]), (200, j + order[2])], 0)
        j += 200
    add("a tie of three at j, j + 1, j + 64: best == second, the ratio is 1", [(7, j), (7, j + 1), (7, j + 64)], None)
    j += 200
    add("a tie for second place behind a clear best at j + 64", [(3, j + 64), (50, j), (50, j + 1)], 0)
    j += 200
    add("a tie for second place that rejects", [(40, j + 1), (50, j), (50, j + 64)], None)
    # no exclusivity: the next two left features share row and descriptor neighbourhood -- built below by copying the descriptor
    add("no exclusivity, first taker", [(4, None), (150, None)], 0)
    c = _stereo_subcases(subs, 61, 4096, "the partner choice among 4096 right features: 0, 1, 2 and 3 candidates around both thresholds, ties, best and second best "
                                          "in one lane and in two, a partner taken twice")
    # a second left feature with the first taker's descriptor, two pixels to its right in the same row: the same partner
    s = len(subs) - 1
    rng = np.random.default_rng(62)
    extra_map = near(rng, c["desc_l"][s], 40)
    c["xy_l"] = np.vstack([c["xy_l"], c["xy_l"][s] + np.float32([2.0, 0.0])]).astype(np.float32)
    c["desc_l"] = np.vstack([c["desc_l"], near(rng, extra_map, 1)[None]])
    c["map_desc"] = np.vstack([c["map_desc"], extra_map[None]])
    c["map_xyz"] = np.vstack([c["map_xyz"], [[1.0, 2.0, 3.0]]])
    inner, expect = c["check"], c["expect"]

    def check(case, ref):
        assert ref["feat"].tolist() == list(range(len(subs) + 1))
        inner(case, dict(ref, feat=ref["feat"][:-1]))
        a, b = partner_of(case, ref, s), partner_of(case, ref, s + 1)
        assert a is not None and b is not None and expect[s] in a and expect[s] in b                          # taken twice
        assert sum(v is None for v in expect.values()) >= 8 and sum(v is not None for v in expect.values()) >= 8
    c["check"] = check
    return c


def all_candidates_case():
    """every one of 4096 right features is a candidate of left feature 0 (its wavefront walks 64 strides with every lane live); feature 1 has the same
    descriptor neighbourhood and takes the same partner; feature 2 lies left of every right feature: no candidate at all"""
    rng = np.random.default_rng(63)
    NR = 4096
    map_desc = rand_desc(rng, 203)
    desc = np.array([near(rng, map_desc[200 + s], 2) for s in range(3)], np.uint8)
    xy = np.array([[1240.5, 200.9], [1239.25, 199.3], [0.5, 200.2]])
    xy_r = np.column_stack([rng.uniform(2.0, 1200.0, NR), rng.uniform(198.0, 201.0, NR)])        # inside both bands: [198, 202] and [197, 201]
    desc_r = rand_desc(rng, NR)
    best, second = 4095, 64 * 31 + 7
    desc_r[best], desc_r[second] = near(rng, desc[0], 6), near(rng, desc[0], 80)                 # (the last lane's last stride; lane 7, stride 31)
    desc[1] = near(rng, desc[0], 30)                                                            # 36 or fewer bits from the best partner, 50 or more from the second
    map_desc[200], map_desc[201] = desc[0], near(rng, desc[1], 1)                               # (feature 0 is nearest to point 200, feature 1 to 201)

    def check(case, ref):
        assert ref["feat"].tolist() == [0, 1, 2] and ref["map_idx"].tolist() == [200, 201, 202]
        assert ref["has_pc"].tolist() == [True, True, False]
        assert best in partner_of(case, ref, 0) and best in partner_of(case, ref, 1)
        x, y = case["right"][0].T
        assert all(_in_band(200.9, v) and _in_band(199.3, v) for v in y) and (np.float32(1239.25) - x >= 1).all() and (np.float32(0.5) - x < 1).all()
    return _case(prm=params(0.75, 0.75), xy_l=xy, desc_l=desc, right=(xy_r, desc_r), map_xyz=rng.normal(0, 10, (203, 3)), map_desc=map_desc, check=check,
                 plants="4096 candidates for one left feature, the same partner for a second, none for a third")


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------------
def _table():
    t = dict(sizes_cases())
    t["B-ratio-0.75-small"] = lambda: accept_case(PAIRS_075[:3], 0.75, 40, "the accept rule at the exact threshold 0.75: (0,0) rejected, (0,5) accepted, (3,4) rejected as equal; in every pass")
    t["B-ratio-0.75-equal"] = lambda: two_point_case(PAIRS_075[3:4], 0.75, 43, "the accept rule at 0.75: (96,128) is equal, rejected; in every pass")
    t["B-ratio-0.75-sides"] = lambda: two_point_case(PAIRS_075[4:], 0.75, 44, "the accept rule at 0.75: (95,128) accepted, (97,128) rejected; in every pass")
    t["B-ratio-default"] = lambda: two_point_case(pairs_at_default(0.8), 0.8, 42, "the accept rule at the default 0.8: the integer pairs nearest fp32(0.8) below, at and above")
    t["B-one-point"] = one_point_case
    for w in (1, 2, 3, 4):
        t[f"C-{'i' * w if w < 4 else 'iv'}"] = lambda w=w: claim_case(w)
    t["D-band-disparity"] = band_case
    t["E-partner-choice"] = partner_case
    t["E-all-candidates"] = all_candidates_case
    for N in (1025, 4096):
        t[f"F-rgbd-N{N}"] = lambda N=N: dict(scene(N, 3300, 70 + N, sensor=2, plants=f"RGB-D, {N} features at fractional coordinates: Pc from the depth for every correspondence"),
                                             check=_check_rgbd)
    t["G-copy1-decoys"] = lambda: dict(scene(1025, 3100, 80, decoys=True, map_copy=1, plants="the map in copy 1; copy 0 holds decoys: every feature's own descriptor, other positions"),
                                       check=_check_decoys)
    t["G-lost-counts"] = lambda: dict(scene(2049, 3100, 81, n_right=1500, decoys=True, lost_frame=1,
                                            plants="a LOST frame's counts: 2049 left and 1500 right features; decoys in copy 1"), check=_check_decoys)
    return t


def _check_rgbd(case, ref):
    assert ref["has_pc"].all() and ref["n_with_point"] == ref["n_corr"] > 0.6 * len(case["xy_l"])
    assert (case["xy_l"] != np.floor(case["xy_l"])).mean() > 0.9
    _check_sizes(case, ref)


def _check_decoys(case, ref):
    _check_sizes(case, ref)
    wrong = restate(dict(case, map_xyz=case["other"][0], map_desc=case["other"][1]))
    n = min(len(case["xy_l"]), len(case["map_xyz"]))
    assert (wrong["records"][:n, 1] == 0).all()                      # the decoys would match better ...
    assert wrong["n_corr"] != ref["n_corr"] and not np.array_equal(wrong["X"][:10], ref["X"][:10])
    assert not np.isin(case["other"][0], case["map_xyz"]).any()       # ... and no position of theirs is one of the map's
    if case["lost_frame"]:
        assert len(case["xy_l"]) == 2049 and len(case["right"][0]) == 1500 and ref["n_with_point"] > 500


CASES = _table()
CASE_NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case_and_answer(name):
    """(case, restate(case)), built once per process and shared: leave both unchanged"""
    case = CASES[name]()
    return case, restate(case)
