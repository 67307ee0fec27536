"""Snapshots of a sequence's state (lvt_amd_snapshot_*): taken while the source goes on, applied to fresh handles and to seats of a lock-step batch, exported
and imported.  A restored tracker continues BIT FOR BIT as its source did -- poses, states, counters, features, matches, map and staged arrays -- and the
source equals the oracle, so every continuation does.  (C_ROW_FALLBACK and the debug stamps say how the streams met, not what was computed: not compared.)"""
import ctypes
import os
import tempfile

import numpy as np
import pytest

from parity_util import make_case, diff_frame, pose_errors, POSE_TOL
from test_gpu_mixed_batch import Seq, run

pytestmark = pytest.mark.gpu

CUTS = (0, 1, 3, 4, 5, 6, 8)    # snapshots of A after this many frames
N_FRAMES = 12


def record(h, R, t, keys):
    """everything a frame leaves behind that the continuation of a restored tracker must repeat"""
    q, p = h.pose()
    c = h.counts()
    rec = {"R": R, "t": t, "q": q, "p": p, "state": h.get_state(), "counts": {k: c[k] for k in keys}}
    for eye in (0, 1):
        rec[f"features{eye}"] = h.features(eye)
    rec["matches"], rec["row_matches"], rec["map"], rec["staged"] = h.matches(), h.row_matches(), h.map(), h.staged()
    return rec


def state_only(rec):
    """what answers from the snapshot as soon as restore() returns"""
    return {k: rec[k] for k in ("q", "p", "state", "counts", "map", "staged")}


def differing(a, b):
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, tuple):
            same = len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y))
        elif isinstance(x, np.ndarray):
            same = np.array_equal(x, y)
        else:
            same = x == y
        if not same:
            bad.append(k)
    return bad


def continue_and_compare(h, ref, k, upto=N_FRAMES):
    """h holds the state after k frames of ref's run: before any frame it answers as A did after frame k - 1, then every frame repeats A's"""
    before = {"q": h.pose()[0], "p": h.pose()[1], "state": h.get_state(), "counts": {n: h.counts()[n] for n in ref["keys"]}, "map": h.map(), "staged": h.staged()}
    assert differing(state_only(ref["recs"][k - 1]), before) == [], (k, differing(state_only(ref["recs"][k - 1]), before))
    for i in range(k, upto):
        R, t = h.track(*ref["frames"][i])
        assert h.last_error() == "", (k, i, h.last_error())
        bad = differing(ref["recs"][i], record(h, R, t, ref["keys"]))
        assert bad == [], f"cut {k}, frame {i}: {bad} differ from the source's"


@pytest.fixture(scope="module")
def ref(hip_lib, oracle_lib):
    """handle A tracks the full-size case synchronously beside one oracle; snapshots are taken after CUTS frames while A goes on.  Computed once, read by
    every test below; recs[-1] is A before any frame."""
    world, prm, sensor = make_case("kitti", 1, 1.0)
    frames = [world.render_stereo(i) for i in range(N_FRAMES)]
    A = hip_lib.LvtSystem.create(prm, sensor)
    orc = oracle_lib.Oracle(prm, sensor)
    keys = [k for k in orc.counts() if k != "row_fallback"]
    out = {"prm": prm, "frames": frames, "keys": keys, "recs": {}, "snaps": {}, "bytes": {}, "info": {}, "msgs": {}, "sizes": []}
    out["recs"][-1] = record(A, np.eye(3), np.zeros(3), keys)
    for i in range(N_FRAMES):
        if i in CUTS:
            s = out["snaps"][i] = A.snapshot()
            out["bytes"][i], out["info"][i] = s.to_bytes(), s.info
            if i == 4:
                again = A.snapshot()                             # a second take of the same state
                out["twice"] = again.to_bytes()
                again.close()
        Ro, to = orc.track(*frames[i])
        Rh, th = A.track(*frames[i])
        msgs = diff_frame(A, orc)
        e_t, e_R = pose_errors(Rh, th, Ro, to)
        if e_t > POSE_TOL or e_R > POSE_TOL:
            msgs.append(f"pose e_t={e_t:.3e} e_R={e_R:.3e}")
        out["msgs"][i] = msgs
        out["recs"][i] = record(A, Rh, th, keys)
        out["sizes"].append((out["recs"][i]["counts"]["map_size"], out["recs"][i]["counts"]["staged_size"]))
    A.close()     # (the snapshots are the library's, not the handle's: they outlive it)
    yield out
    for s in out["snaps"].values():
        s.close()


def test_continuation_is_bit_identical_and_equals_the_oracle(hip_lib, ref):
    print("map / staged sizes per frame:", ref["sizes"])
    print("cuts:", {k: (i["state"], i["map_n"], i["staged_n"], i["src_map_cur"], i["src_staged_cur"]) for k, i in ref["info"].items()})
    assert all(m == [] for m in ref["msgs"].values()), ref["msgs"]
    info = ref["info"]
    # the cuts are not trivial states: an empty one, a staged set with counters in flight (the next frame promotes 100 of its 188 points), every residue
    # of the 16-byte copies, both ping-pong copies of the map and of the staged set as the live one
    assert (info[0]["state"], info[0]["map_n"], info[0]["staged_n"], info[0]["frame_number"]) == (1, 0, 0, 0)
    assert (info[4]["map_n"], info[4]["staged_n"]) == (721, 188) and ref["recs"][4]["counts"]["n_staged_promoted"] == 100
    assert {info[k]["staged_n"] % 4 for k in CUTS} >= {0, 2, 3} and {info[k]["staged_n"] for k in CUTS} >= {188, 174, 35}
    assert {info[k]["map_n"] % 4 for k in CUTS} >= {1, 3} and {info[k]["map_n"] for k in CUTS} >= {721, 851}
    assert {info[k]["src_map_cur"] for k in CUTS} == {0, 1} and {info[k]["src_staged_cur"] for k in CUTS} == {0, 1}
    for k in CUTS:
        assert info[k]["bytes"] == len(ref["bytes"][k]) and info[k]["sensor_type"] == 1 and info[k]["state"] == (2 if k else 1)
        assert bytes(ref["snaps"][k].params.to_pod()) == bytes(ref["prm"].to_pod())
        B = hip_lib.LvtSystem.create(ref["prm"], 1)
        assert B.restore(ref["snaps"][k]) == 0, B.last_error()
        continue_and_compare(B, ref, k)
        B.close()


def test_a_snapshot_behind_frames_in_flight_equals_the_synchronous_one(hip_lib, ref):
    """five frames enqueued through lvt_amd_track_async, none collected: take drains, and the bytes are those of the synchronous run's cut"""
    A = hip_lib.LvtSystem.create(ref["prm"], 1)
    for i in range(5):
        assert A.track_async(*ref["frames"][i]) == 0, A.last_error()
    assert A.host_stats()["collected"] == 0
    got = A.snapshot().to_bytes()
    assert A.last_error() == ""
    assert got == ref["bytes"][5], [i for i in range(0, len(got), 4) if got[i:i + 4] != ref["bytes"][5][i:i + 4]][:16]
    A.close()


def test_bytes(hip_lib, ref):
    S = hip_lib.Snapshot
    raw = ref["bytes"][4]
    assert ref["twice"] == raw                                   # two takes of one state
    info, prm = S.describe(raw)
    assert info == dict(ref["info"][4], device=-1) and bytes(prm.to_pod()) == bytes(ref["prm"].to_pod())
    imported = S.from_bytes(raw)
    assert imported.to_bytes() == raw
    B = hip_lib.LvtSystem.create(ref["prm"], 1)
    assert B.restore(imported) == 0, B.last_error()
    assert B.snapshot().to_bytes() == raw                        # taken directly after the restore: the applied bytes
    continue_and_compare(B, ref, 4)
    B.close()
    flipped = bytearray(raw); flipped[len(raw) // 2] ^= 0x10     # a payload byte
    version = bytearray(raw); version[8] ^= 0x02                 # the version field
    def poke(at):                                                # one header field changed (k_state.hip, SnapHeader: 32-bit fields from byte 8 on)
        b = bytearray(raw); b[at] ^= 0x04
        return bytes(b)
    for bad, word in ((bytes(flipped), "checksum"), (raw[:-1], "truncated"), (raw[:100], "too short"), (bytes(version), "version"), (poke(0), "magic"),
                      (poke(16), "another build"), (poke(24), "capacities"), (poke(37), "offsets"), (poke(157), "offsets")):
        for call in (S.from_bytes, S.describe):
            with pytest.raises(ValueError) as e:
                call(bad)
            assert word in str(e.value), (word, str(e.value))


def test_clone(hip_lib, ref):
    """one snapshot applied to two handles (one of them beside a live handle: it orders its streams with events): both continue as A did"""
    B1, B2 = hip_lib.LvtSystem.create(ref["prm"], 1), hip_lib.LvtSystem.create(ref["prm"], 1)
    assert B1.restore(ref["snaps"][4]) == 0 and B2.restore(ref["snaps"][4]) == 0, (B1.last_error(), B2.last_error())
    for i in range(4, 8):
        r1 = record(B1, *B1.track(*ref["frames"][i]), ref["keys"])
        r2 = record(B2, *B2.track(*ref["frames"][i]), ref["keys"])
        assert differing(r1, r2) == [] and differing(ref["recs"][i], r1) == [], (i, differing(r1, r2), differing(ref["recs"][i], r1))
    B1.close(); B2.close()


def check_seats(batch, seqs, schedule, got, orcs):
    """test_gpu_mixed_batch.check_against_own_oracles with the oracles handed in (a seat that arrives by snapshot brings an oracle that has tracked already)"""
    for s, q in enumerate(seqs):
        for k, which in enumerate(schedule):
            if which[s] is None:
                continue
            Ro, to = orcs[s].track(*q.frames[which[s]])
            Rb, tb, st = got[k]
            e_t, e_R = pose_errors(Rb[s], tb[s], Ro, to)
            print(f"sequence {s} step {k} frame {which[s]}: e_t {e_t:.2e} e_R {e_R:.2e} state {st[s]} / {orcs[s].status}")
            assert e_t <= POSE_TOL and e_R <= POSE_TOL and st[s] == orcs[s].status, f"sequence {s} step {k}: {e_t:.2e} {e_R:.2e} state {st[s]} oracle {orcs[s].status}"


def counters_equal(batch, s, orc):
    co, ch = orc.counts(), batch.counts(s)
    bad = {k: (ch.get(k), v) for k, v in co.items() if ch.get(k) != v}
    assert not bad, f"sequence {s}: counters (hip, oracle) {bad}"


def test_into_and_out_of_a_mixed_batch(hip_lib, oracle_lib):
    """a drive that started on a handle of its own joins a running batch; later a seat leaves it for a handle of its own"""
    sizes = ((1241, 376), (1242, 375), (1226, 370))
    seqs = []
    for s, size in enumerate(sizes):
        world, prm, _ = make_case("kitti", 60 + s, 1.0, None, size=size)
        seqs.append(Seq(world, prm, 16 if s == 2 else 12))
    orcs = [oracle_lib.Oracle(q.prm, 1) for q in seqs]
    batch = hip_lib.LvtBatch.create_mixed([q.prm for q in seqs])
    first = [[i, None, i] for i in range(5)]
    got = run(batch, seqs, first)
    solo = hip_lib.LvtSystem.create(seqs[1].prm, 1)
    for i in range(5):
        Ro, to = orcs[1].track(*seqs[1].frames[i])
        Rh, th = solo.track(*seqs[1].frames[i])
        assert max(pose_errors(Rh, th, Ro, to)) <= POSE_TOL and solo.get_state() == orcs[1].status
    snap = solo.snapshot()
    assert batch.restore(1, snap) == 0, batch.last_error()       # (run() has collected every step: the batch is idle)
    co, ch = orcs[1].counts(), batch.counts(1)
    assert all(ch[k] == v for k, v in co.items()), (co, ch)      # seat 1 answers from the snapshot at once
    solo.close(); snap.close()
    rest = [[i, i, i] for i in range(5, 12)]
    got += run(batch, seqs, rest)
    assert batch.last_error() == "", batch.last_error()
    check_seats(batch, seqs, first + rest, got, orcs)
    for s in range(3):
        counters_equal(batch, s, orcs[s])
    snaps = batch.snapshot()                                     # every seat through one drain and one launch
    assert [x.info["map_n"] for x in snaps] == [batch.counts(s)["map_size"] for s in range(3)]
    out = hip_lib.LvtSystem.create(seqs[2].prm, 1)
    assert out.restore(snaps[2]) == 0, out.last_error()
    for i in range(12, 16):                                      # the only place where the arrays that come out of a batch seat are compared
        Ro, to = orcs[2].track(*seqs[2].frames[i])
        Rh, th = out.track(*seqs[2].frames[i])
        assert diff_frame(out, orcs[2]) == [] and max(pose_errors(Rh, th, Ro, to)) <= POSE_TOL, (i, diff_frame(out, orcs[2]))
    out.close()
    for x in snaps:
        x.close()


def test_a_batch_with_more_snapshots_than_one_table_holds(hip_lib):
    """a uniform batch of 17 (sequence s starts at frame s % 3 of the half-size world) is snapshot after two steps -- a second k_state_pack launch, whose table
    holds sequence 16 alone --, exported, imported and applied to a second batch of 17 -- a second k_state_unpack launch.  Sequences 0, 15 and 16 export the bytes
    a solo handle on the same frames exports, and continue in the second batch with the solo handle's poses bit for bit, as every sequence does with the first batch's"""
    world, prm, _ = make_case("kitti", 0, 0.5)
    B, cut, n = 17, 2, 4
    q = Seq(world, prm, n + 2)
    solo = {}
    for o in (0, 1):                                             # (sequences 0 and 15 start at frame 0, sequence 16 at frame 1)
        h = hip_lib.LvtSystem.create(prm, 1)
        for i in range(cut):
            h.track(*q.frames[o + i])
        snap = h.snapshot()
        solo[o] = (snap.to_bytes(), [h.track(*q.frames[o + i]) for i in range(cut, n)])
        assert h.last_error() == "" and h.get_state() == 2, h.last_error()
        snap.close(); h.close()

    def steps(batch, ks):
        out = []
        for k in ks:
            fr = [q.ptrs(k + s % 3) for s in range(B)]
            batch.track_device_async([f[0] for f in fr], [f[1] for f in fr], q.H, q.W, q.pitch)
            out.append(batch.wait())
            assert batch.last_error() == "", batch.last_error()
        return out

    first = hip_lib.LvtBatch(prm, B)
    steps(first, range(cut))
    snaps = first.snapshot()
    raw = [x.to_bytes() for x in snaps]
    for s in (0, 15, 16):
        want = solo[s % 3][0]
        assert raw[s] == want, (s, [i for i in range(0, len(want), 4) if raw[s][i:i + 4] != want[i:i + 4]][:16])
    second = hip_lib.LvtBatch(prm, B)
    imported = [hip_lib.Snapshot.from_bytes(b) for b in raw]
    assert second.restore_all(imported) == 0, second.last_error()
    for s in (0, 15, 16):
        assert second.counts(s) == first.counts(s), s              # (the seats answer from the snapshots at once)
    a, b = steps(first, range(cut, n)), steps(second, range(cut, n))
    for k in range(n - cut):
        assert list(b[k][2]) == [2] * B, (k, list(b[k][2]))
        assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]), f"step {cut + k}: the restored batch's poses differ from the source's"
        for s in (0, 15, 16):
            R, t = solo[s % 3][1][k]
            assert np.array_equal(b[k][0][s], R) and np.array_equal(b[k][1][s], t), f"sequence {s} step {cut + k}: not the solo handle's pose"
    for x in snaps + imported:
        x.close()
    first.close(); second.close()


def test_rgbd(hip_lib, oracle_lib):
    world, prm, sensor = make_case("tum", 0, 1.0)
    assert sensor == 2
    frames = [world.render_rgbd(i) for i in range(7)]
    A, orc = hip_lib.LvtSystem.create(prm, 2), oracle_lib.Oracle(prm, 2)
    for i in range(3):
        orc.track_rgbd(*frames[i]); A.track(*frames[i])
    assert diff_frame(A, orc) == []
    snap = A.snapshot()
    assert (snap.info["sensor_type"], snap.info["staged_n"], snap.info["map_n"]) == (2, 0, orc.counts()["map_size"]) and snap.info["map_n"] > 600
    A.close()
    B = hip_lib.LvtSystem.create(prm, 2)
    assert B.restore(snap) == 0, B.last_error()
    for i in range(3, 7):
        Ro, to = orc.track_rgbd(*frames[i])
        Rh, th = B.track(*frames[i])
        assert diff_frame(B, orc) == [] and max(pose_errors(Rh, th, Ro, to)) <= POSE_TOL, (i, diff_frame(B, orc))
    B.close(); snap.close()


def test_lost_and_reset_of_one_sequence(hip_lib, oracle_lib):
    """seat 1 of three goes LOST on two flat images; its snapshot is LOST on a handle of its own; reset(1) re-initialises it alone"""
    import torch
    n = 14
    cases = (("kitti", 70, 1.0, (621, 187)), ("kitti", 0, 0.5, None), ("kitti", 72, 1.0, (613, 185)))
    seqs = []
    for kind, seed, scale, size in cases:
        world, prm, _ = make_case(kind, seed, scale, None, size=size)
        seqs.append(Seq(world, prm, n))
    q1 = seqs[1]
    assert (q1.W, q1.H) == (620, 188)
    flat = np.full((q1.H, q1.W), 110, np.uint8)
    for i in (4, 5):
        q1.frames[i] = (flat, flat)
        q1.dev[i, :, :, :q1.W] = 110
    torch.cuda.synchronize()
    orcs = [oracle_lib.Oracle(q.prm, 1) for q in seqs]
    batch = hip_lib.LvtBatch.create_mixed([q.prm for q in seqs])
    schedule = [[i, i, i] for i in range(n)]
    got = run(batch, seqs, schedule[:6])
    assert [int(g[2][1]) for g in got] == [2, 2, 2, 2, 3, 3]
    # the LOST seat on a handle of its own: LOST there too, and the next frame returns the last pose, as an oracle that is not reset does
    lost_orc = oracle_lib.Oracle(q1.prm, 1)
    for i in range(7):
        Ro, to = lost_orc.track(*q1.frames[i])
    assert lost_orc.status == 3
    snap = batch.snapshot(1)
    assert snap.info["state"] == 3
    solo = hip_lib.LvtSystem.create(q1.prm, 1)
    assert solo.restore(snap) == 0 and solo.get_state() == 3, solo.last_error()
    Rh, th = solo.track(*q1.frames[6])
    assert solo.get_state() == 3 and max(pose_errors(Rh, th, Ro, to)) <= POSE_TOL
    assert np.array_equal(Rh, got[5][0][1]) and np.array_equal(th, got[5][1][1])
    solo.close(); snap.close()
    assert batch.reset(1) == 0, batch.last_error()
    got += run(batch, seqs, schedule[6:])
    assert batch.last_error() == "", batch.last_error()
    assert [int(g[2][1]) for g in got[6:]] == [2] * 8
    assert np.array_equal(got[6][0][1], np.eye(3)) and not got[6][1][1].any()
    for s in (0, 1, 2):                                           # seats 0 and 2 against their uninterrupted oracles, seat 1 against one reset before frame 6
        for k in range(n):
            if s == 1 and k == 6:
                orcs[1].reset()
            Ro, to = orcs[s].track(*seqs[s].frames[k])
            e_t, e_R = pose_errors(got[k][0][s], got[k][1][s], Ro, to)
            assert e_t <= POSE_TOL and e_R <= POSE_TOL and got[k][2][s] == orcs[s].status, (s, k, e_t, e_R, got[k][2][s], orcs[s].status)
        counters_equal(batch, s, orcs[s])
    assert batch.counts(1)["map_size"] > 150 and orcs[0].status == orcs[2].status == 2


def test_refusals_change_nothing(hip_lib, oracle_lib):
    import torch
    L = hip_lib.load_library()
    vp = ctypes.c_void_p
    world, prm, _ = make_case("kitti", 0, 0.5)
    frames = [world.render_stereo(i) for i in range(4)]
    H, orc = hip_lib.LvtSystem.create(prm, 1), oracle_lib.Oracle(prm, 1)
    for i in range(2):
        orc.track(*frames[i]); H.track(*frames[i])
    good = H.snapshot()

    def refused(rc, handle, *words):
        why = handle.last_error()
        assert rc in (-1, None) and why and all(w in why for w in words), (rc, why, words)

    # seq out of range, the batch calls on a solo handle
    refused(L.lvt_amd_snapshot_take(vp(H._h), 1), H, "no sequence 1")
    refused(L.lvt_amd_snapshot_apply(vp(H._h), 2, vp(good._h)), H, "no sequence 2")
    one = (vp * 1)(good._h)
    refused(L.lvt_amd_batch_snapshot_take(vp(H._h), one), H, "not a batch")
    refused(L.lvt_amd_batch_snapshot_apply(vp(H._h), one), H, "not a batch")
    refused(L.lvt_amd_batch_reset(vp(H._h), 0), H, "not a batch")
    # other parameters, another sensor type
    _, other, _ = make_case("kitti", 0, 0.5, {"tracking_radius": 30})
    X = hip_lib.LvtSystem.create(other, 1)
    sx = X.snapshot()
    refused(H.restore(sx), H, "parameters differ")
    D = hip_lib.LvtSystem.create(prm, 2)
    sd = D.snapshot()
    refused(H.restore(sd), H, "sensor type")
    for x in (X, D, sx, sd):
        x.close()
    # another device
    if torch.cuda.device_count() > 1:
        far = hip_lib.Snapshot.from_bytes(good.to_bytes(), device=1)
        assert far.info["device"] == 1
        refused(H.restore(far), H, "device 1")
        far.close()
    # a batch names the sequence
    batch = hip_lib.LvtBatch.create_mixed([prm, other])
    refused(batch.restore(2, good), batch, "no sequence 2")
    refused(batch.restore(1, good), batch, "sequence 1", "parameters differ")
    refused(batch.restore_all([good, good]), batch, "sequence 1", "parameters differ")
    assert batch.counts(0)["map_size"] == 0                      # (sequence 0 was not applied either)
    refused(batch.reset(2), batch, "no sequence 2")
    with pytest.raises(RuntimeError):
        batch.snapshot(2)
    batch.close()
    # frames in flight
    assert H.track_async(*frames[2]) == 0
    refused(H.restore(good), H, "frames in flight")
    Ro, to = orc.track(*frames[2])
    Rh, th, st = H.wait_status()
    assert st == orc.status == 2 and max(pose_errors(Rh, th, Ro, to)) <= POSE_TOL
    # the refusals have changed nothing: the next frame still equals the oracle
    Ro, to = orc.track(*frames[3])
    Rh, th = H.track(*frames[3])
    msgs = diff_frame(H, orc)
    assert msgs[:1] == ["hip error: " + H.last_error()] and "frames in flight" in msgs[0]    # (a refusal's report stays until the next report)
    assert msgs[1:] == [] and max(pose_errors(Rh, th, Ro, to)) <= POSE_TOL, msgs
    # pooled and automatic seats, both ways
    P, porc = hip_lib.LvtSystem.create(prm, 1, pooled=True), oracle_lib.Oracle(prm, 1)
    porc.track(*frames[0]); P.track(*frames[0])
    refused(L.lvt_amd_snapshot_take(vp(P._h), 0), P, "pooled")
    refused(P.restore(good), P, "pooled")
    Ro, to = porc.track(*frames[1])
    Rh, th = P.track(*frames[1])
    assert max(pose_errors(Rh, th, Ro, to)) <= POSE_TOL and P.get_state() == porc.status == 2
    P.close()
    cfg = os.path.join(tempfile.mkdtemp(), "cfg.yaml")
    prm.write_yaml(cfg)
    a1, a2 = hip_lib.LvtSystem.create_from_file(cfg, 1), hip_lib.LvtSystem.create_from_file(cfg, 1)
    assert a1.ordering() == a2.ordering() == "pooled"            # (automatic seats: two unused lvt_create handles with the same parameters)
    for a in (a1, a2):
        refused(L.lvt_amd_snapshot_take(vp(a._h), 0), a, "seat")
        refused(a.restore(good), a, "seat")
    a1.close(); a2.close()
    H.close(); good.close()
