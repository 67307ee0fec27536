"""LABEL MASKS on the GPU: lvt_amd_set_label_mask, lvt_amd_frame_labels / _device, the launch k_label_mask at the head of the feature stage, plane 8, and the
stage entry lvt_amd_build_label_mask.  No expected value comes from this library: the definition is restated in numpy (label_mask_util.label_plane, held to
hand-checked answers and to its literal reading by test_label_masks.py), and the tracker is held to the UNCHANGED oracle fed that frame's numpy plane through
the two equivalences of mask_util -- stereo: the oracle's external-corner route with its detector's corners filtered by the plane; RGB-D: the depth zeroed
under the plane.  Every oracle chain is asserted TRACKING and every compared frame drops at least 10 % of its features.  The sequences run on the sliding labels
at QUARTER resolution with dilate 3, where the previous frame's labels decide at least 5 features of every frame differently (test_label_masks.py asserts it):
a frame filtered with its neighbour's labels cannot pass.  The worlds: kitti 71 at 621 x 187 (the left eye labelled) and tum 0 at 322 x 242, 8 frames."""
import ctypes as C

import numpy as np
import pytest

import label_mask_util as LU
import mask_util as MU
from parity_util import make_case, diff_frame
from test_gpu_raw_frames import close_to, counts_equal, get_case, _run_async as run_async
from test_gpu_colour_frames import device_colour, device_gray, assert_plane
from test_gpu_feature_masks import stereo, rgbd, Follow, _profile_of

pytestmark = pytest.mark.gpu

N = LU.N_FRAMES
DILATE = 3


# ---- 1. the stage entry against numpy, byte for byte -------------------------------------------------------------------------------------------
def label_sizes(W, H):
    return [(W, H), ((W + 3) // 4, (H + 3) // 4), (100, 37), (2 * W, 2 * H), (1, 1)]


def contents(LW, LH, seed):
    """(name, label image, drop set): all allowed, all forbidden, a forbidden label pixel in each corner, random labels under a random drop set, isolated
    forbidden pixels at three densities (their dilation windows cross every tile edge)"""
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, 256, (LH, LW)).astype(np.uint8)
    corners = np.zeros((LH, LW), np.uint8)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = 200
    out = [("all allowed", rnd, []), ("all forbidden", rnd, list(range(256))), ("corners", corners, [200]),
           ("random", rnd, [int(l) for l in np.flatnonzero(rng.random(256) < 0.3)])]
    for k, den in enumerate((50, 500, 5000)):
        iso = np.where(np.random.default_rng(1000 + den).random((LH, LW)) < 1.0 / den, 255, k).astype(np.uint8)
        out.append((f"isolated 1/{den}", iso, [255]))
    return out


def padded(a, pitch, offset, fill):
    """`a` as a view into rows of `pitch` bytes that starts `offset` bytes past a 16-byte boundary; every other byte holds `fill`"""
    H, W = a.shape
    store = np.full(16 + offset + H * pitch + 16, fill, np.uint8)
    base = (-store.ctypes.data) % 16 + offset
    v = np.lib.stride_tricks.as_strided(store[base:], shape=(H, W), strides=(pitch, 1))
    v[:] = a
    assert v.ctypes.data % 16 == offset % 16 and v.strides[0] == pitch
    return v


def check_stage(hip_lib, W, H, sizes, dilates, pick, out_pitches):
    n = 0
    for si, (LW, LH) in enumerate(sizes):
        for name, lab, drop in contents(LW, LH, 7 * W + si):
            if not pick(name):
                continue
            # a label pitch above the width and an odd address; the padding holds a FORBIDDEN label where the set has one: a wrong pitch or address would show
            fill = drop[0] if drop else 0
            view = padded(lab, LW + 5, 1 + 2 * (n % 2), fill)
            for d in dilates:
                for with_static in (False, True):
                    static = None
                    if with_static:
                        static = padded(np.where(np.random.default_rng(n).random((H, W)) < 0.9, 1 + n % 255, 0).astype(np.uint8), W + 3, 3, 255)
                    out_pitch = out_pitches[n % len(out_pitches)]
                    want = LU.label_plane(lab, drop, d, W, H, static)
                    got = hip_lib.build_label_mask(hip_lib.LabelMask(LW, LH, drop, d), view, W, H, static, out_pitch)
                    assert_plane(got, want, W, H, out_pitch, f"{W} x {H}, labels {LW} x {LH}, {name}, dilate {d}, static {with_static}, out pitch {out_pitch}")
                    n += 1
    return n


@pytest.mark.parametrize("W,H", [(33, 17), (64, 32), (65, 33), (322, 242)])
def test_stage_entry_equals_numpy_byte_for_byte(hip_lib, W, H):
    """the smallest images that carry a seam and a ragged edge of the 32 x 32 tile, and one TUM-shaped; every label size, dilation, content and layout; output
    pitches of 64-byte multiples and of the width rounded up to 4 (a last tile column that is part plane, part nothing)"""
    n = check_stage(hip_lib, W, H, label_sizes(W, H), (0, 1, 3, 15), lambda name: True, ((W + 63) // 64 * 64, (W + 3) // 4 * 4))
    assert n == 5 * 7 * 4 * 2


def test_stage_entry_on_a_kitti_sized_image(hip_lib):
    n = check_stage(hip_lib, 1241, 376, [((1241 + 3) // 4, (376 + 3) // 4), (100, 37)], (0, 15), lambda name: name in ("random", "isolated 1/500", "isolated 1/5000"), (1280,))
    assert n == 2 * 3 * 2 * 2


def test_stage_entry_leaves_the_bytes_around_the_output_alone(hip_lib):
    """guard bytes before and behind the host plane come back untouched (on the device the plane stands between guard bytes the entry checks itself)"""
    W, H, pitch = 65, 33, 68
    lab = np.random.default_rng(3).integers(0, 4, (9, 17)).astype(np.uint8)
    rec = hip_lib.LabelMask(17, 9, [1], 3)
    store = np.full(64 + H * pitch + 64, 0x77, np.uint8)
    rc = hip_lib.load_library().lvt_amd_build_label_mask(C.byref(rec), lab.ctypes.data_as(C.c_void_p), 17, W, H, None, 0, C.c_void_p(store.ctypes.data + 64), pitch)
    assert rc == 0, hip_lib.load_library().lvt_amd_last_error(None)
    assert np.all(store[:64] == 0x77) and np.all(store[64 + H * pitch:] == 0x77)
    assert_plane(store[64:64 + H * pitch].reshape(H, pitch), LU.label_plane(lab, [1], 3, W, H), W, H, pitch, "the guarded plane")


# ---- inputs of the sequences ---------------------------------------------------------------------------------------------------------------------
_ONCE = {}


def sliding(q, dilate=DILATE, static=None, key=None):
    """(record, [label image], [numpy plane]) of the sliding sequence at quarter resolution on q's image"""
    k = (id(q), dilate, key)
    if k not in _ONCE:
        size = LU.label_sizes(q.W, q.H)["quarter"]
        labs, masks = LU.sliding_masks(q.W, q.H, size, dilate, static)
        _ONCE[k] = (size, labs, masks)
    size, labs, masks = _ONCE[k]
    import lvt_amd
    return lvt_amd.LabelMask(size[0], size[1], LU.DROPPED, dilate), labs, masks


def labelled_system(hip_lib, q, rec, sensor=1):
    hip = hip_lib.LvtSystem.create(q.prm, sensor)
    assert hip.set_label_mask(rec) == 0, hip.last_error()
    got = hip.label_mask()
    assert (got.label_width, got.label_height, got.dilate, got.dropped()) == (rec.label_width, rec.label_height, rec.dilate, rec.dropped())
    return hip


def chain(q, left, right, n=N):
    """the oracle over the first n stereo frames, frame i under the planes left[i] / right[i] (None: none): ([(R, t, state, counts)], oracle, responses)"""
    k = ("chain", id(q), id(left), id(right), n)
    if k not in _ONCE:
        orc, out, resp = q.oracle(), [], None
        for i in range(n):
            R, t, resp = MU.oracle_track_masked(orc, q.prm, *q.frames[i], left[i], right[i] if right else None, f"frame {i}", 0.10 if left[i] is not None else 0.0)
            out.append((np.array(R), np.array(t), orc.status, orc.counts()))
        assert [r[2] for r in out] == [2] * n, "the oracle is not TRACKING on every frame"
        _ONCE[k] = (out, orc, resp, left, right)   # (the lists are kept: their ids name the entry)
    return _ONCE[k][:3]


def check_async(q, hip, got, left, right):
    ref, orc, resp = chain(q, left, right, len(got))
    for i, (R, t, st) in enumerate(got):
        assert st == ref[i][2], f"frame {i}: state {st} oracle {ref[i][2]}"
        close_to(R, t, ref[i], f"frame {i}")
    msgs = MU.diff_frame_but_resp(hip, orc, resp)
    assert not msgs, msgs[:6]
    counts_equal(hip.counts(), ref[len(got) - 1][3], "last frame")


def stats_of(corners_xy, mask):
    k = MU.keep_rule(corners_xy[:, 0], corners_xy[:, 1], mask)
    return int(k.sum()), int((~k).sum())


# ---- 2. the synchronous host call, statistics and plane 8 ------------------------------------------------------------------------------------------
def test_stereo_sequence_through_lvt_track(hip_lib, oracle_lib):
    """labels for the left eye before every lvt_track; every frame against the oracle, lvt_amd_get_mask_stats and plane 8 against numpy"""
    q = stereo()
    rec, labs, masks = sliding(q)
    hip, f = labelled_system(hip_lib, q, rec), Follow(q)
    assert hip.mask_stats() is None and hip.plane(0, 8).size == 0
    for i in range(N):
        assert hip.frame_labels(labs[i], None) == 0, hip.last_error()
        Ro, to = f.frame(i, masks[i], None, 0.10)
        R, t = hip.track(*q.frames[i])
        f.hold(hip, i, R, t, Ro, to)
        assert_plane(hip.plane(0, 8), masks[i], q.W, q.H, q.pitch, f"frame {i}: plane 8")
        assert hip.plane(1, 8).size == 0
        st, c = hip.mask_stats(), hip.counts()
        assert st["kept"] == (c["n_left"], 0) and st["dropped"][0] > 0 and st["dropped"][1] == 0, st
        before = MU.border_kept(MU.masked_corners(q.frames[i][0], q.prm, None)[0], q.W, q.H)
        assert (st["kept"][0], st["dropped"][0]) == stats_of(before, masks[i]), (i, st)


# ---- 3. frames in flight: where the binding shows --------------------------------------------------------------------------------------------------
def test_three_frames_in_flight_through_track_async(hip_lib, oracle_lib):
    """lvt_amd_track_async holds every frame back until the next one arrives: the labels of frame i are attached while frame i - 1 is held and frames before
    it are in flight.  A build that bound them to the held frame, or to the slot instead of the frame, filters with a neighbour's labels"""
    q = stereo()
    rec, labs, masks = sliding(q)
    hip = labelled_system(hip_lib, q, rec)

    def submit(i):
        assert hip.frame_labels(labs[i], None) == 0, hip.last_error()
        if i:
            assert hip.host_stats()["enqueued"] > hip.host_stats()["collected"], "no frame in flight while the labels were attached"
        assert hip.track_async(*q.frames[i]) == 0, hip.last_error()
    got = run_async(hip, submit, N, 3)
    assert hip.last_error() == "", hip.last_error()
    check_async(q, hip, got, masks, None)
    assert_plane(hip.plane(0, 8), masks[N - 1], q.W, q.H, q.pitch, "the last frame's plane")


def test_device_planes_at_an_odd_pitch_three_in_flight(hip_lib, oracle_lib):
    """frames and labels in HBM: the label planes lie 1 byte past an aligned address, rows label_width + 7 bytes apart, every other byte holding a FORBIDDEN
    label; both eyes labelled (the right eye with the labels of the frame four later)"""
    q = stereo()
    rec, labs, masks = sliding(q)
    hip = labelled_system(hip_lib, q, rec)
    right = [masks[(i + 4) % N] for i in range(N)]
    keep = [[device_colour(labs[j][:, :, None], 1, extra=7, guard=13) for j in (i, (i + 4) % N)] for i in range(N)]
    assert keep[0][0][1] % 2 == 1 and keep[0][0][2] == rec.label_width + 7
    dev = [device_gray([f[e] for f in q.frames], q.W, q.H, q.pitch) for e in (0, 1)]

    def submit(i):
        (_, pl, pitch), (_, pr, _) = keep[i]
        assert hip.frame_labels(pl, pr, pitch, pitch) == 0, hip.last_error()
        hip.track_device_async(dev[0][i].data_ptr(), dev[1][i].data_ptr(), q.H, q.W, q.pitch)
    got = run_async(hip, submit, N, 3)
    assert hip.last_error() == "", hip.last_error()
    check_async(q, hip, got, masks, right)
    for eye, m in enumerate((masks, right)):
        assert_plane(hip.plane(eye, 8), m[N - 1], q.W, q.H, q.pitch, f"eye {eye}")


# ---- 4. the other routes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "async"])
def test_rgbd_frames(hip_lib, oracle_lib, route):
    from oracle import pyoracle as O
    q = rgbd()
    rec, labs, masks = sliding(q)
    hip, orc = labelled_system(hip_lib, q, rec, 2), q.oracle()
    for i in range(N):
        g, d = q.frames[i]
        MU.dropped_share(O.detect_grid(g, q.prm)[0], masks[i], f"frame {i}", 0.10)
        Ro, to = orc.track_rgbd(g, MU.masked_depth(d, masks[i]))
        assert hip.frame_labels(labs[i]) == 0, hip.last_error()
        if route == "host":
            R, t = hip.track(g, d)
        else:
            assert hip.track_async(g, d) == 0, hip.last_error()
            R, t, _ = hip.wait_status()
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        assert_plane(hip.plane(0, 8), masks[i], q.W, q.H, q.pitch, f"frame {i}: plane 8")


def test_external_corners(hip_lib, oracle_lib):
    """lvt_track_with_external_corners: the tracker is given every corner of the oracle's detector and the labels, the oracle the corners the plane keeps"""
    from oracle import pyoracle as O
    q = stereo()
    rec, labs, masks = sliding(q)
    hip, orc = labelled_system(hip_lib, q, rec), q.oracle()
    for i in range(N):
        cl, cr = (O.detect_grid(a, q.prm)[0][:, :2].astype(np.float64) for a in q.frames[i])
        kl = MU.filter_corners(cl, masks[i])
        assert len(kl) < 0.95 * len(cl)
        Ro, to = orc.track_with_external_corners(*q.frames[i], kl, cr)
        assert hip.frame_labels(labs[i], None) == 0, hip.last_error()
        R, t = hip.track_with_external_corners(*q.frames[i], cl, cr)
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")


def test_with_a_static_bonnet_mask_as_well(hip_lib, oracle_lib):
    """the bonnet on both eyes, labels on the left: the left plane is the AND of both, the right eye is filtered by the bonnet alone"""
    q = stereo()
    bonnet = q.masks["bonnet"]
    rec, labs, masks = sliding(q, static=bonnet, key="bonnet")
    assert any(np.any((m == 0) & (bonnet != 0)) for m in masks)
    hip, f = labelled_system(hip_lib, q, rec), Follow(q)
    assert hip.set_mask(bonnet, bonnet) == 0, hip.last_error()
    for i in range(N):
        assert hip.frame_labels(labs[i], None) == 0, hip.last_error()
        Ro, to = f.frame(i, masks[i], bonnet, 0.10)
        R, t = hip.track(*q.frames[i])
        f.hold(hip, i, R, t, Ro, to)
        assert_plane(hip.plane(0, 8), masks[i], q.W, q.H, q.pitch, f"frame {i}: plane 8")
        st = hip.mask_stats()
        assert min(st["dropped"]) > 0 and st["kept"] == (hip.counts()["n_left"], hip.counts()["n_right"]), st


def test_with_rectifiers_the_labels_live_on_the_rectified_grid(hip_lib, oracle_lib):
    """raw frames in, labels on the grid the detector reads: the oracle is fed the oracle-rectified frames and ITS corners on them filtered by the plane"""
    c = get_case("A")
    rec, labs, masks = sliding(c)
    hip = hip_lib.LvtSystem.create(c.prm, 1)
    rl, rr = c.rectifiers(hip_lib)
    assert hip.set_rectifiers(rl, rr) == 0 and hip.set_label_mask(rec) == 0, hip.last_error()
    orc = c.oracle()
    for i in range(4):
        Ro, to, resp = MU.oracle_track_masked(orc, c.prm, *c.rect[i], masks[i], None, f"frame {i}", 0.10)
        assert hip.frame_labels(labs[i], None) == 0, hip.last_error()
        R, t = hip.track(*c.raw[i])
        assert orc.status == 2
        msgs = MU.diff_frame_but_resp(hip, orc, resp)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")


# ---- 5. a frame without labels, replace, clear, reset ------------------------------------------------------------------------------------------------
def test_no_labels_replace_clear_and_reset(hip_lib, oracle_lib):
    """frame 2 gets no labels; frame 3's labels are attached twice (the wrong ones first); frame 4's are attached and cleared again; frame 5's are attached,
    then lvt_amd_reset drops them and the frame goes in unlabelled as the first of a fresh chain; frames 6 and 7 are labelled again.  An attachment is consumed
    by ITS frame alone: frames 2 and 4 behind labelled ones are filtered by nothing"""
    q = stereo()
    rec, labs, masks = sliding(q)
    hip, f = labelled_system(hip_lib, q, rec), Follow(q)
    plan = [masks[0], masks[1], None, masks[3], None, None, masks[6], masks[7]]
    for i in range(N):
        if i in (0, 1, 6, 7):
            assert hip.frame_labels(labs[i], None) == 0, hip.last_error()
        if i == 3:
            assert hip.frame_labels(labs[0], labs[0]) == 0 and hip.frame_labels(labs[3], None) == 0, hip.last_error()
        if i == 4:
            assert hip.frame_labels(labs[4], None) == 0 and hip.frame_labels(None, None) == 0, hip.last_error()
        if i == 5:
            assert hip.frame_labels(labs[5], None) == 0, hip.last_error()
            hip.reset()
            f = Follow(q)
            assert hip.label_mask() is not None, "a reset took the record"
        Ro, to = f.frame(i, plan[i], None, 0.10 if plan[i] is not None else 0.0)
        R, t = hip.track(*q.frames[i])
        f.hold(hip, i, R, t, Ro, to)
        assert (hip.mask_stats() is None) == (plan[i] is None) and (hip.plane(0, 8).size == 0) == (plan[i] is None), i


# ---- 6. a mixed batch ----------------------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_labels_a_static_mask_and_an_absent_sequence(hip_lib, oracle_lib):
    """three sequences, three steps in flight: 0 = 621 x 187 with labels on the left eye in every step; 1 = 613 x 185 under a static bonnet alone; 2 = 621 x 187
    with a record, labelled in every step it takes part in -- and ALSO handed labels (all forbidden) for steps 2 and 4, which it sits out: the step consumes
    them, the frame of the step behind is filtered by its own.  Sequences 0 and 2 against the oracle chains, sequence 1 against a solo handle"""
    q = stereo()
    rec, labs, masks = sliding(q)
    bw, bprm, _ = make_case("kitti", 32, size=(613, 185))
    bframes = [tuple(np.ascontiguousarray(a) for a in bw.render_stereo(i)) for i in range(6)]
    bpitch, bonnet = 640, MU.bonnet(613, 185)
    batch = hip_lib.LvtBatch([q.prm, bprm, q.prm])
    assert batch.set_label_mask(0, rec) == 0 and batch.set_label_mask(2, rec) == 0 and batch.set_mask(1, bonnet, bonnet) == 0, batch.last_error()
    assert batch.label_mask(1) is None and batch.label_mask(2).dilate == DILATE
    dev = [device_gray([f[e] for f in q.frames], q.W, q.H, q.pitch) for e in (0, 1)]
    devb = [device_gray([f[e] for f in bframes], 613, 185, bpitch) for e in (0, 1)]
    forbidden = np.full_like(labs[0], 13)
    nsteps, which, f2 = 6, [], 0
    for k in range(nsteps):
        which.append([k, k, None if k in (2, 4) else f2])
        f2 += 0 if k in (2, 4) else 1

    def ptr(s, i, e):
        return None if i is None else (devb if s == 1 else dev)[e][i].data_ptr()
    got, inflight = [], 0
    for k in range(nsteps):
        assert batch.frame_labels(0, labs[k], None) == 0, batch.last_error()
        assert batch.frame_labels(2, forbidden if which[k][2] is None else labs[which[k][2]], None) == 0, batch.last_error()
        rc = batch.track_device_async_mixed([ptr(s, which[k][s], 0) for s in range(3)], [ptr(s, which[k][s], 1) for s in range(3)], [q.H, 185, q.H],
                                            [q.W, 613, q.W], [q.pitch, bpitch, q.pitch])
        assert rc == 0, batch.last_error()
        inflight += 1
        if inflight >= 3:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    assert batch.last_error() == "", batch.last_error()
    for s in (0, 2):
        steps = [k for k in range(nsteps) if which[k][s] is not None]
        ref, _, _ = chain(q, masks, None, len(steps))
        for j, k in enumerate(steps):
            R, t, st = got[k]
            assert st[s] == ref[j][2] == 2, f"sequence {s} step {k}: state {st[s]}"
            close_to(R[s], t[s], ref[j], f"sequence {s} step {k}")
        counts_equal(batch.counts(s), ref[len(steps) - 1][3], f"sequence {s} after the last step")
        assert batch.mask_stats(s)["dropped"][0] > 0 and batch.mask_stats(s)["dropped"][1] == 0
    solo = hip_lib.LvtSystem.create(bprm, 1)
    assert solo.set_mask(bonnet, bonnet) == 0
    for k in range(nsteps):
        solo.track_device_async(devb[0][k].data_ptr(), devb[1][k].data_ptr(), 185, 613, bpitch)
        R, t, st = solo.wait_status()
        assert st == got[k][2][1] == 2 and np.array_equal(R, got[k][0][1]) and np.array_equal(t, got[k][1][1]), f"sequence 1 step {k}"
    assert batch.mask_stats(1) == solo.mask_stats()


# ---- 7. launch accounting and snapshots ---------------------------------------------------------------------------------------------------------------
def test_launch_accounting_and_snapshot_bytes(hip_lib, oracle_lib):
    """a handle with neither property has no k_label_mask and no k_mask_features row; a handle with a record and labels adds exactly those two, one call per
    labelled frame, every other row as the plain one; a frame without labels launches neither; the snapshot bytes do not know the record"""
    q = stereo()
    rec, labs, masks = sliding(q)
    full = hip_lib.LabelMask(rec.label_width, rec.label_height, [], 0)   # nothing is dropped: the same frames as the plain handle
    plain = hip_lib.LvtSystem.create(q.prm, 1)
    plain.profile_enable(True)
    for i in range(4):
        plain.track(*q.frames[i])
    rows = _profile_of(plain)
    assert rows and not [n for n, _ in rows if "mask" in n], rows
    plain_bytes = plain.snapshot().to_bytes()
    plain.close()
    hip = labelled_system(hip_lib, q, full)
    hip.profile_enable(True)
    for i in range(4):
        assert hip.frame_labels(labs[i], None) == 0
        hip.track(*q.frames[i])
    prof = _profile_of(hip)
    assert dict(prof)["k_label_mask"] == 4 and dict(prof)["k_mask_features"] == 4, prof
    assert [(n, k) for n, k in prof if n not in ("k_label_mask", "k_mask_features")] == rows, (prof, rows)
    assert hip.mask_stats()["dropped"] == (0, 0)
    assert hip.snapshot().to_bytes() == plain_bytes, "the snapshot of a handle with a label-mask record knows it"
    hip.track(*q.frames[4])
    prof = dict(_profile_of(hip))
    assert prof["k_label_mask"] == 4 and prof["k_mask_features"] == 4, "a frame without labels still launches"
    assert hip.set_label_mask(None) == 0 and hip.label_mask() is None


# ---- 8. every refusal, in the contract's order -------------------------------------------------------------------------------------------------------
U, A = " (nothing was changed)", " (nothing was attached)"
RIDES = "a pooled handle (its frames ride a chain shared with other handles)"
SET, LAB, DEV = "lvt_amd_set_label_mask: ", "lvt_amd_frame_labels: ", "lvt_amd_frame_labels_device: "
TEXT = {
    "pooled": SET + RIDES + U,
    "solo call on a batch": SET + "a batch handle takes its label masks per sequence through lvt_amd_batch_set_label_mask" + U,
    "batch call on a solo": SET + "lvt_amd_batch_set_label_mask on a handle that is not a batch (use lvt_amd_set_label_mask)" + U,
    "seq 2": SET + "no sequence 2 in this handle" + U,
    "width": SET + "a label mask with label_width = 0 (1 ... 8192)" + U,
    "height": SET + "a label mask with label_height = 8193 (1 ... 8192)" + U,
    "dilate": SET + "a label mask with dilate = 16 (0 ... 15)" + U,
    "in flight": SET + "frames in flight: set the label mask before the first frame or after every frame has been collected" + U,
    "labels pooled": LAB + RIDES + A,
    "labels seq 1": LAB + "no sequence 1 in this handle" + A,
    "labels no record": LAB + "a sequence without a label-mask record: set one with lvt_amd_set_label_mask first" + A,
    "labels pitch": DEV + "a label pitch of 155 bytes on label images 156 pixels wide (pitch >= label_width)" + A,
    "labels right eye": LAB + "right-eye labels on an RGB-D handle (it has one image: pass NULL for the right eye)" + A,
}


def test_every_refusal_says_its_sentence(hip_lib, oracle_lib, tmp_path):
    """each refusal returns -1 and leaves its complete sentence; where two objections apply the earlier one of the contract's order is named; a refused
    attachment attaches nothing, and the handle goes on tracking against the oracle"""
    q, r = stereo(), rgbd()
    rec, labs, masks = sliding(q)
    assert rec.label_width == 156
    L, seen = hip_lib.load_library(), []

    def refused(h, rc, key):
        assert rc == -1 and h.last_error() == TEXT[key], (key, rc, h.last_error())
        seen.append(key)

    def bad(**kw):
        b = hip_lib.LabelMask(rec.label_width, rec.label_height, LU.DROPPED, DILATE)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    hip, f = hip_lib.LvtSystem.create(q.prm, 1), Follow(q)
    refused(hip, hip.frame_labels(labs[0], None), "labels no record")
    refused(hip, L.lvt_amd_frame_labels(hip._h, 1, None, None), "labels seq 1")                      # the sequence before the record
    refused(hip, L.lvt_amd_batch_set_label_mask(hip._h, 0, C.byref(rec)), "batch call on a solo")
    refused(hip, L.lvt_amd_batch_set_label_mask(hip._h, 5, C.byref(bad(dilate=16))), "batch call on a solo")   # the spelling before the sequence and the record
    refused(hip, hip.set_label_mask(bad(label_width=0)), "width")
    refused(hip, hip.set_label_mask(bad(label_height=8193, dilate=16)), "height")
    refused(hip, hip.set_label_mask(bad(dilate=16)), "dilate")
    assert hip.label_mask() is None
    assert hip.set_label_mask(rec) == 0, hip.last_error()
    dl = device_colour(labs[1][:, :, None], 0, extra=3)
    refused(hip, hip.frame_labels(dl[1], 0, 155, 0), "labels pitch")
    refused(hip, hip.frame_labels(dl[1], dl[1], dl[2], 155), "labels pitch")
    # frames in flight: the record is refused (the record before the frames in flight), the labels are accepted
    dev = device_gray(list(q.frames[0]), q.W, q.H, q.pitch)
    assert hip.frame_labels(labs[0], None) == 0
    hip.track_device_async(dev[0].data_ptr(), dev[1].data_ptr(), q.H, q.W, q.pitch)
    refused(hip, hip.set_label_mask(bad(dilate=16)), "dilate")
    refused(hip, hip.set_label_mask(None), "in flight")
    assert hip.frame_labels(labs[1], None) == 0, hip.last_error()
    refused(hip, hip.frame_labels(dl[1], 0, 155, 0), "labels pitch")      # refused: the attachment made before it stands
    Ro, to = f.frame(0, masks[0], None)
    R, t, st = hip.wait_status()
    assert st == 2
    close_to(R, t, (Ro, to), "frame 0")
    Ro, to = f.frame(1, masks[1], None)
    R, t = hip.track(*q.frames[1])
    said = hip.last_error()   # (the last refusal's sentence stays until the next report)
    msgs = [x for x in MU.diff_frame_but_resp(hip, f.orc, f.resp) if x != "hip error: " + said]
    assert not msgs and f.orc.status == 2, msgs[:6]
    close_to(R, t, (Ro, to), "frame 1")
    hip.close()

    rg = hip_lib.LvtSystem.create(r.prm, 2)
    rr = hip_lib.LabelMask(8, 8, [1], 0)
    assert rg.set_label_mask(rr) == 0, rg.last_error()
    z = np.zeros((8, 8), np.uint8)
    refused(rg, rg.frame_labels(z, z), "labels right eye")
    refused(rg, rg.frame_labels(None, z), "labels right eye")
    rg.close()

    batch = hip_lib.LvtBatch(q.prm, 2)
    refused(batch, L.lvt_amd_set_label_mask(batch._h, C.byref(rec)), "solo call on a batch")
    refused(batch, batch.set_label_mask(2, bad(dilate=16)), "seq 2")                                   # the sequence before the record
    assert batch.set_label_mask(1, rec) == 0 and batch.label_mask(0) is None
    assert batch.frame_labels(0, labs[0], None) == -1 and batch.last_error() == TEXT["labels no record"]
    with pytest.raises(IndexError):
        batch.label_mask(2)
    batch.close()

    seat = hip_lib.LvtSystem.create(q.prm, 1, pooled=True)
    q.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    autos = [hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1) for _ in range(2)]
    assert seat.ordering() == "pooled" and autos[0].ordering() == "pooled"
    for h in (seat, autos[0]):
        refused(h, h.set_label_mask(bad(dilate=16)), "pooled")                                         # the kind before everything
        refused(h, L.lvt_amd_frame_labels(h._h, 3, None, None), "labels pooled")
        assert h.label_mask() is None
    for h in [seat] + autos:
        h.close()
    assert set(seen) == set(TEXT), set(TEXT) - set(seen)
