"""FRAME REDUCTION on the GPU: the stage entry (lvt_amd_reduce_device) against the numpy restatement byte for byte, and reduced sequences against the UNCHANGED
oracle, which is fed the numpy-reduced frames and the reduced intrinsics (reduce_util).  No expected value comes from the library under test.  Frames in
flight together are held to the oracle by state and pose, frame by frame, and by the complete parity_util.diff_frame behind the last one; the synchronous
routes run diff_frame behind every frame."""
import itertools

import numpy as np
import pytest

import colour_util as CU
import reduce_util as RU
from parity_util import diff_frame
from test_gpu_raw_frames import close_to, counts_equal, _run_async as run_async

pytestmark = pytest.mark.gpu

GUARD = 0xA5
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65)
HEIGHTS = (1, 2, 3, 17)
OFFSETS = (0, 1, 2, 3, 8, 16)


# ---- the stage entry -----------------------------------------------------------------------------------------------------------------------------
def stage(hip_lib, src, f, offset=0, src_pitch=None, dst_extra=0, pad=255):
    """src (h, w) u8 through lvt_amd_reduce_device.  The source lies `offset` bytes past a 256-byte boundary, rows src_pitch apart, every byte that is no pixel
    holds `pad`; the destination has dst_pitch = the reduced width rounded up to 4, + dst_extra, and GUARD bytes in front of and behind it.  Returns the
    destination rows (h // f, dst_pitch) after checking the guards."""
    import torch
    sh, sw = src.shape
    w, h = sw // f, sh // f
    src_pitch = sw if src_pitch is None else src_pitch
    dst_pitch = (w + 3) // 4 * 4 + dst_extra
    d0 = 256
    s0 = (d0 + h * dst_pitch + 256 + 255) // 256 * 256 + offset
    buf = np.full(s0 + sh * src_pitch + 64, pad, np.uint8)
    buf[:s0 - offset] = GUARD
    np.lib.stride_tricks.as_strided(buf[s0:], shape=(sh, sw), strides=(src_pitch, 1))[:] = src
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 256 == 0
    rc, launches = hip_lib.reduce_device(t.data_ptr() + s0, sw, sh, src_pitch, f, t.data_ptr() + d0, dst_pitch)
    assert (rc, launches) == (0, 1), hip_lib.last_call_error()
    out = t.cpu().numpy()
    assert (out[:d0] == GUARD).all() and (out[d0 + h * dst_pitch:s0 - offset] == GUARD).all(), "guard bytes around the destination were written"
    assert np.array_equal(out[s0 - offset:], buf[s0 - offset:]), "the source was written"
    return out[d0:d0 + h * dst_pitch].reshape(h, dst_pitch)


def check(hip_lib, src, f, what, **kw):
    got = stage(hip_lib, src, f, **kw)
    want = RU.reduce(src, f)
    w = want.shape[1]
    bad = np.argwhere(got[:, :w] != want)
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at {tuple(bad[0])}: hip {got[tuple(bad[0])]} numpy {want[tuple(bad[0])]}"
    assert not got[:, w:].any(), f"{what}: the padding columns are not zero"


def placements(sw):
    """(offset, pitch) of a source sw bytes wide: every offset with an odd pitch and with a multiple of 16 -- offsets 0, 8, 16 with the latter take the
    vector path, everything else the byte path"""
    for off in OFFSETS:
        yield off, (sw + 1) | 1
        yield off, (sw + 15) // 16 * 16 + 16


@pytest.mark.parametrize("f", range(2, 9))
def test_stage_sizes_trailing_pixels_and_placements(hip_lib, f):
    """every destination width and height of the lists, every count 0 ... f - 1 of trailing source columns and rows, planted with 255 over a dark image (as is
    every byte between the rows): anything read beyond f bW of a row or below row f bH - 1 shows in the result.  The placements rotate through the cases"""
    rng = np.random.default_rng(100 + f)
    n = 0
    for w, h in itertools.product(WIDTHS, HEIGHTS):
        for tc, tr in itertools.product(range(f), range(f)):
            src = np.full((f * h + tr, f * w + tc), 255, np.uint8)
            src[:f * h, :f * w] = rng.integers(0, 16, size=(f * h, f * w), dtype=np.uint8)
            pl = list(placements(src.shape[1]))
            off, pitch = pl[n % len(pl)]
            check(hip_lib, src, f, f"f {f} w {w} h {h} trailing {tc} x {tr} offset {off} pitch {pitch}", offset=off, src_pitch=pitch, dst_extra=4 * (n % 3))
            n += 1


@pytest.mark.parametrize("f", range(2, 9))
def test_stage_vector_and_byte_paths_give_the_same_bytes(hip_lib, f):
    """one random image, 65 x 17 reduced with f - 1 trailing columns and rows, at every offset and both kinds of pitch"""
    src = np.random.default_rng(f).integers(0, 256, size=(f * 17 + f - 1, f * 65 + f - 1), dtype=np.uint8)
    for off, pitch in placements(src.shape[1]):
        check(hip_lib, src, f, f"f {f} offset {off} pitch {pitch}", offset=off, src_pitch=pitch)


@pytest.mark.parametrize("f", range(2, 9))
def test_stage_contents(hip_lib, f):
    """all 0, all 255, the checkerboard of 0 / 255 (the ties) and the EVERY-SUM image -- blocks whose sums take every value 0 ... 255 f f: the proof of the
    division -- on the vector path and on the byte path"""
    yy, xx = np.mgrid[0:f * 9, 0:f * 13]
    images = {"zeros": np.zeros((f * 9, f * 13), np.uint8), "ones": np.full((f * 9, f * 13), 255, np.uint8),
              "checkerboard": (((yy + xx) & 1) * 255).astype(np.uint8), "every sum": RU.every_sum_image(f)}
    for name, img in images.items():
        for off in (0, 1):
            check(hip_lib, img, f, f"f {f} {name} offset {off}", offset=off, src_pitch=(img.shape[1] + 15) // 16 * 16)


def test_stage_refusals(hip_lib):
    import torch
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    for args, word in (((0, 16, 16, 16, 2, p, 8), "NULL"), ((p, 16, 16, 16, 1, p + 1024, 8), "factor"), ((p, 16, 16, 16, 9, p + 1024, 8), "factor"),
                       ((p, 1, 16, 16, 2, p + 1024, 8), "source side"), ((p, 16, 16, 15, 2, p + 1024, 8), "source pitch"),
                       ((p, 16, 16, 16, 2, p + 1024, 4), "destination"), ((p, 16, 16, 16, 2, p + 1024, 10), "destination"), ((p, 16, 16, 16, 2, p + 1025, 8), "destination")):
        assert hip_lib.reduce_device(*args) == (-1, 0), args
        assert word in hip_lib.last_call_error() and hip_lib.last_call_error().endswith("(nothing was launched)"), hip_lib.last_call_error()


# ---- sequences -------------------------------------------------------------------------------------------------------------------------------------
def kitti2():
    return RU.large_world("kitti", 3, (1240, 376), 2)


def kitti3():
    return RU.large_world("kitti", 3, (1241, 376), 3)


def reduced_system(hip_lib, q, prm=None):
    hip = hip_lib.LvtSystem.create(prm or q.prm, q.sensor)
    assert hip.set_reduction(q.reduction()) == 0, hip.last_error()
    r = hip.reduction()
    assert (r.factor, r.width, r.height) == (q.f, q.fW, q.fH)
    return hip


def device_plane(img, offset, extra=5, guard=255):
    """a gray image in HBM `offset` bytes past an aligned address, rows W + extra bytes apart, `guard` everywhere else: (owner, address, pitch)"""
    import torch
    H, W = img.shape
    pitch = W + extra
    buf = np.full(256 + offset + H * pitch + 256, guard, np.uint8)
    np.lib.stride_tricks.as_strided(buf[256 + offset:], shape=(H, W), strides=(pitch, 1))[:] = img
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + 256 + offset, pitch


def assert_plane(p, want, what):
    H, W = want.shape
    assert p.dtype == np.uint8 and p.shape[0] == H and p.shape[1] >= W and p.shape[1] % 64 == 0, (what, p.shape)
    bad = np.argwhere(p[:, :W] != want)
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at {tuple(bad[0])}: hip {p[tuple(bad[0])]} numpy {want[tuple(bad[0])]}"
    assert not p[:, W:].any(), f"{what}: the padding columns are not zero"


def sync_sequence(hip, orc, n, large, small, after=None):
    for i in range(n):
        Ro, to = orc.track(*small(i))
        R, t = hip.track(*large(i))
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        if after:
            after(i)


def check_async(q, hip, got, small=None):
    ref = q.chain(range(len(got)), images=small)
    for i, (R, t, st) in enumerate(got):
        assert st == ref[i][2], f"frame {i}: state {st} oracle {ref[i][2]}"
        close_to(R, t, ref[i], f"frame {i}")
    orc = q.oracle()
    for i in range(len(got)):
        orc.track(*(small or q.small)[i])
    msgs = diff_frame(hip, orc)
    assert not msgs, msgs[:6]


def test_lvt_track_on_pageable_buffers(hip_lib, oracle_lib):
    """kitti 620 x 188 from 1240 x 376 through lvt_track, six frames; plane 9 of every frame is the numpy reduction and planes 2 / 3 stay empty"""
    q = kitti2()
    hip = reduced_system(hip_lib, q)

    def after(i):
        for eye in (0, 1):
            assert_plane(hip.plane(eye, 9), q.small[i][eye], f"frame {i} eye {eye}")
        assert hip.plane(0, 2).size == 0 and hip.plane(0, 3).size == 0
    sync_sequence(hip, q.oracle(), 6, lambda i: q.large[i], lambda i: q.small[i], after)


def test_track_async_three_in_flight(hip_lib, oracle_lib):
    q = kitti2()
    hip = reduced_system(hip_lib, q)

    def submit(i):
        assert hip.track_async(*q.large[i]) == 0, hip.last_error()
    got = run_async(hip, submit, 6, 3)
    check_async(q, hip, got)
    hs = hip.host_stats()
    assert hs["async_host_frames"] == 6 and hs["pulls_carried_by_the_previous_frame"] > 0, hs


def test_device_planes_at_an_odd_address_and_pitch(hip_lib, oracle_lib):
    q = kitti2()
    hip = reduced_system(hip_lib, q)
    dev = [[device_plane(img, 1 + (i + e) % 3) for e, img in enumerate(q.large[i])] for i in range(6)]
    assert dev[0][0][2] % 2 == 1

    def submit(i):
        hip.track_device_async(dev[i][0][1], dev[i][1][1], q.fH, q.fW, dev[i][0][2])
    got = run_async(hip, submit, 6, 3)
    assert hip.last_error() == "", hip.last_error()
    check_async(q, hip, got)


def test_factor_three_with_trailing_columns(hip_lib, oracle_lib):
    """kitti 413 x 125 from 1241 x 376: two trailing columns, one trailing row"""
    q = kitti3()
    assert (q.fW - 3 * q.W, q.fH - 3 * q.H) == (2, 1)
    sync_sequence(reduced_system(hip_lib, q), q.oracle(), 5, lambda i: q.large[i], lambda i: q.small[i])


def test_rgb8_frames_convert_then_reduce(hip_lib, oracle_lib):
    q = kitti2()
    chan = [[CU.colour_channels(g, 3, i, eye) for eye, g in enumerate(q.large[i])] for i in range(4)]
    gray = [tuple(np.ascontiguousarray(CU.gray_of_rgb(*c[:3])) for c in pair) for pair in chan]
    small = [tuple(RU.reduce(g, 2) for g in pair) for pair in gray]
    hip = reduced_system(hip_lib, q)
    assert hip.set_pixel_format(CU.RGB8) == 0, hip.last_error()

    def after(i):
        if i == 0:
            for eye in (0, 1):
                assert_plane(hip.plane(eye, 3), gray[0][eye], f"converted, eye {eye}")     # (frame-sized)
                assert_plane(hip.plane(eye, 9), small[0][eye], f"reduced, eye {eye}")
    sync_sequence(hip, q.oracle(), 4, lambda i: tuple(CU.pack(*c, CU.RGB8) for c in chan[i]), lambda i: small[i], after)


def test_rectifiers_and_reduction_together(hip_lib, oracle_lib):
    """a calibration of the full-size raw image: lvt_amd_lens_reduced gives the lens of the reduced image, the rectifier's source.  Full-size raw frame ->
    reduce -> remap; the numpy chain is reduce_util + lens_util + remap_util"""
    import lens_util as LU
    from remap_util import remap
    q = kitti2()
    w = q.world
    full = hip_lib.Lens(LU.RADTAN, q.fW, q.fH, [[w.fx, 0, w.cx], [0, w.fy, w.cy], [0, 0, 1]], [0.03, -0.01, 1e-4, -1e-4, 0.002])
    lens = full.reduced(2)
    P = [[q.prm.fx, 0, q.prm.cx], [0, q.prm.fy, q.prm.cy], [0, 0, 1]]
    m1, m2 = LU.lens_maps(lens.model, lens.K, lens.D, np.eye(3), P, q.W, q.H)
    rect = [tuple(np.ascontiguousarray(remap(s, m1, m2)[0]) for s in pair) for pair in q.small[:4]]
    hip = hip_lib.LvtSystem.create(q.prm, 1)
    r = hip_lib.Rectifier.from_lens(lens, np.eye(3), P, q.W, q.H)
    assert hip.set_rectifiers(r, r) == 0, hip.last_error()           # rectifiers first, then the reduction
    assert hip.set_reduction(q.reduction()) == 0, hip.last_error()

    def after(i):
        if i == 0:
            for eye in (0, 1):
                assert_plane(hip.plane(eye, 9), q.small[0][eye], f"reduced, eye {eye}")
                assert_plane(hip.plane(eye, 2), rect[0][eye], f"rectified, eye {eye}")
    sync_sequence(hip, q.oracle(), 4, lambda i: q.large[i], lambda i: rect[i], after)


def test_reduction_and_equalisation_together(hip_lib, oracle_lib):
    import clahe_util as CL
    q = kitti2()
    eq = [tuple(np.ascontiguousarray(CL.clahe(s, (8, 4), 3.0)) for s in pair) for pair in q.small[:4]]
    hip = reduced_system(hip_lib, q)
    assert hip.set_equalisation(tiles=(8, 4), clip_limit=3.0) == 0, hip.last_error()
    sync_sequence(hip, q.oracle(), 4, lambda i: q.large[i], lambda i: eq[i])


def test_rgbd_with_a_full_size_depth_camera(hip_lib, oracle_lib):
    """tum 320 x 240 from 640 x 480: the full-size depth enters through a depth camera with identity extrinsics and the full-size pinhole; the oracle is fed
    depth_reg_util's plane"""
    import depth_reg_util as DR
    from test_frame_reduction import full_size_depth_camera
    q = RU.large_world("tum", 3, (640, 480), 2)
    cam = full_size_depth_camera(q)
    hip = reduced_system(hip_lib, q)
    assert hip.set_depth_camera(cam) == 0, hip.last_error()
    orc = q.oracle()
    for i in range(5):
        Ro, to = orc.track_rgbd(q.small[i], DR.register(cam, q.prm, q.depth[i]))
        R, t = hip.track(q.large[i], q.depth[i])
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
    assert_plane(hip.plane(0, 9), q.small[4], "last frame")


def test_mixed_batch_of_two_factors_a_plain_sequence_and_an_absent_one(hip_lib, oracle_lib):
    """0 = f 2; 1 = f 3; 2 = plain (the reduced frames of sequence 0, one frame ahead, as ordinary gray planes); 3 = f 2, sitting out steps 1 and 3.  Each
    against its own oracle chain: state and pose of every step it has a frame in, all counters behind the last"""
    import torch
    a, b = kitti2(), kitti3()
    prms = [a.prm, b.prm, a.prm, a.prm]
    batch = hip_lib.LvtBatch(prms)
    assert batch.set_reduction(0, a.reduction()) == 0 and batch.set_reduction(1, b.reduction()) == 0 and batch.set_reduction(3, a.reduction()) == 0, batch.last_error()
    assert batch.reduction(2) is None and batch.reduction(1).factor == 3
    nsteps = 5
    which = [[k, k, k + 1, None] for k in range(nsteps)]
    f3 = 0
    for k in range(nsteps):
        if k not in (1, 3):
            which[k][3] = f3
            f3 += 1
    images = [a.small, b.small, a.small, a.small]
    devl = {0: [[device_plane(img, 1 + e) for e, img in enumerate(a.large[i])] for i in range(6)],
            1: [[device_plane(img, 2 + e, extra=3) for e, img in enumerate(b.large[i])] for i in range(6)]}
    plain = torch.zeros((6, 2, a.H, a.pitch), dtype=torch.uint8, device="cuda")
    for i in range(6):
        for e in (0, 1):
            plain[i, e, :, :a.W] = torch.from_numpy(a.small[i][e]).cuda()

    def ptrs(s, i):
        if s == 2:
            return plain[i, 0].data_ptr(), plain[i, 1].data_ptr(), a.pitch
        d = devl[1 if s == 1 else 0][i]
        return d[0][1], d[1][1], d[0][2]
    rows, cols = [a.fH, b.fH, a.H, a.fH], [a.fW, b.fW, a.W, a.fW]
    got, inflight = [], 0
    for k in range(nsteps):
        p = [None if which[k][s] is None else ptrs(s, which[k][s]) for s in range(4)]
        rc = batch.track_device_async_mixed([x and x[0] for x in p], [x and x[1] for x in p], rows, cols, [x[2] if x else 0 for x in p])
        assert rc == 0, batch.last_error()
        inflight += 1
        if inflight >= 3:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    assert batch.last_error() == "", batch.last_error()
    from oracle import pyoracle as O
    for s in range(4):
        orc = O.Oracle(prms[s], 1)
        for k in range(nsteps):
            if which[k][s] is None:
                continue
            Ro, to = orc.track(*images[s][which[k][s]])
            R, t, st = got[k]
            assert orc.status == 2, f"sequence {s} step {k}: the oracle is not TRACKING"
            assert st[s] == orc.status, f"sequence {s} step {k}: state {st[s]}"
            close_to(R[s], t[s], (np.array(Ro), np.array(to)), f"sequence {s} step {k}")
        counts_equal(batch.counts(s), orc.counts(), f"sequence {s} after the last step")


def test_a_batch_with_more_reduced_images_than_one_table_holds(hip_lib, oracle_lib):
    """33 reduced stereo sequences = 66 images: the step takes a second k_reduce_frames launch.  Sequence s starts at frame s of one cached world; three
    steps; counts and poses of EVERY sequence against its oracle chain"""
    B, steps = 33, 3
    q = kitti2()
    batch = hip_lib.LvtBatch(q.prm, B)
    for s in range(B):
        assert batch.set_reduction(s, q.reduction()) == 0, batch.last_error()
    dev = [[device_plane(img, 1 + (i + e) % 3) for e, img in enumerate(q.large[i])] for i in range(B + steps - 1)]
    refs = [q.chain(range(s, s + steps)) for s in range(B)]
    batch.profile_enable(True)
    for k in range(steps):
        fr = [dev[k + s] for s in range(B)]
        batch.track_device_async([f[0][1] for f in fr], [f[1][1] for f in fr], q.fH, q.fW, dev[0][0][2])
        R, t, st = batch.wait()
        assert batch.last_error() == "", batch.last_error()
        for s in range(B):
            ref = refs[s][k]
            assert st[s] == ref[2] == 2, (s, k, st[s])
            close_to(R[s], t[s], ref, f"sequence {s} step {k}")
            counts_equal(batch.counts(s), ref[3], f"sequence {s} step {k}")
    assert dict(profile_of(batch))["k_reduce_frames"] == steps   # (the slot times a step's first launch)


# ---- launches, switching, state --------------------------------------------------------------------------------------------------------------------
def profile_of(h):
    return [(name, calls) for name, _ms, calls in h.profile_read()]


def test_profile_slot_launch_count_and_factor_one(hip_lib, oracle_lib):
    """a plain handle has no k_reduce_frames row; a reduced one reports exactly one call per frame and nothing else changes; a handle that set a reduction,
    tracked a large frame, was reset and set factor 1 tracks the small frames to the oracle's bits with the plain handle's launches"""
    q = kitti2()
    plain = hip_lib.LvtSystem.create(q.prm, 1)
    plain.profile_enable(True)
    for i in range(4):
        plain.track(*q.small[i])
    rows = profile_of(plain)
    assert rows and not [n for n, _ in rows if "k_reduce_frames" in n], rows
    assert dict(rows)["k_score"] == 4
    plain.close()   # (a handle created beside a live one orders its streams with events: other rows)

    hip = reduced_system(hip_lib, q)
    hip.profile_enable(True)
    for i in range(4):
        hip.track(*q.large[i])
    prof = profile_of(hip)
    assert dict(prof)["k_reduce_frames"] == 4, prof
    assert [(n, k) for n, k in prof if n != "k_reduce_frames"] == rows, (prof, rows)
    hip.close()

    back = reduced_system(hip_lib, q)
    back.track(*q.large[0])
    back.reset()
    assert back.set_reduction(factor=1, width=q.fW, height=q.fH) == 0, back.last_error()
    assert back.reduction() is None
    back.profile_enable(True)
    orc = q.oracle()
    for i in range(4):
        orc.track(*q.small[i])
        back.track(*q.small[i])
        msgs = diff_frame(back, orc)
        assert not msgs, (i, msgs[:6])
        assert back.plane(0, 9).size == 0
    assert profile_of(back) == rows, (profile_of(back), rows)


def test_snapshots_do_not_hold_the_property_and_reset_leaves_it(hip_lib, oracle_lib):
    q = kitti2()
    plain, hip = hip_lib.LvtSystem.create(q.prm, 1), reduced_system(hip_lib, q)
    for i in range(3):
        plain.track(*q.small[i])
        hip.track(*q.large[i])
    a, b = plain.snapshot(), hip.snapshot()
    assert a.to_bytes() == b.to_bytes()
    assert plain.restore(b) == 0, plain.last_error()
    assert plain.reduction() is None                       # (a snapshot taken from a reduced handle brings no reduction)
    assert hip.restore(a) == 0 and hip.reduction().factor == 2   # (... and one from a plain handle takes none away)
    a.close(); b.close()
    hip.reset()
    r = hip.reduction()
    assert r is not None and (r.factor, r.width, r.height) == (2, q.fW, q.fH)
    sync_sequence(hip, q.oracle(), 3, lambda i: q.large[i], lambda i: q.small[i])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_the_contracts_order(hip_lib, oracle_lib, tmp_path):
    import torch
    q = kitti2()
    L = hip_lib.load_library()
    said = []

    def refused(h, rc, *words):
        assert rc == -1 and h.last_error().endswith("(nothing was changed)"), (rc, h.last_error())
        for w in words:
            assert w in h.last_error(), (w, h.last_error())
        said.append(h.last_error())

    hip, orc = hip_lib.LvtSystem.create(q.prm, 1), q.oracle()
    nxt = [0]

    def next_frame(large=False):
        i = nxt[0]
        nxt[0] += 1
        Ro, to = orc.track(*q.small[i])
        R, t = hip.track(*(q.large[i] if large else q.small[i]))
        msgs = [m for m in diff_frame(hip, orc) if not (said and m == "hip error: " + said[-1])]
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")

    R = hip_lib.Reduction
    # the handle's kind
    seat = hip_lib.LvtSystem.create(q.prm, 1, pooled=True)
    refused(seat, seat.set_reduction(R(9, 0, 0)), "pooled")                                   # (ahead of the value)
    q.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    autos = [hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1) for _ in range(2)]
    assert autos[0].ordering() == "pooled"
    refused(autos[0], autos[0].set_reduction(q.reduction()), "pooled")
    assert seat.reduction() is None
    seat.close()
    for h in autos:
        h.close()
    # the spelling
    refused(hip, L.lvt_amd_batch_set_reduction(hip._h, 5, C_byref(R(9, 0, 0))), "lvt_amd_batch_set_reduction on a handle that is not a batch")
    batch = hip_lib.LvtBatch(q.prm, 2)
    refused(batch, L.lvt_amd_set_reduction(batch._h, C_byref(R(9, 0, 0))), "lvt_amd_batch_set_reduction")
    # seq
    for seq in (-1, 2):
        refused(batch, batch.set_reduction(seq, R(9, 0, 0)), f"no sequence {seq}")
        with pytest.raises(IndexError):
            batch.reduction(seq)
    # the value
    refused(hip, L.lvt_amd_set_reduction(hip._h, None), "NULL")
    for bad in (0, 9, -2):
        refused(hip, hip.set_reduction(R(bad, q.fW, q.fH)), f"factor = {bad}", "(1 ... 8)")
    refused(hip, hip.set_reduction(R(2, 0, q.fH)), "width = 0")
    refused(hip, hip.set_reduction(R(2, 16385, q.fH)), "width = 16385")
    refused(hip, hip.set_reduction(R(2, q.fW, 0)), "height = 0")
    refused(hip, hip.set_reduction(R(2, q.fW + 2, q.fH)), f"{q.W + 1} x {q.H}", f"{q.W} x {q.H}")
    refused(hip, hip.set_reduction(R(3, q.fW, q.fH)), f"{q.fW // 3} x {q.fH // 3}")
    next_frame()
    # frames in flight, behind the value
    dev = torch.zeros((2, q.H, q.pitch), dtype=torch.uint8, device="cuda")
    for e in (0, 1):
        dev[e, :, :q.W] = torch.from_numpy(q.small[nxt[0]][e]).cuda()
    hip.track_device_async(dev[0].data_ptr(), dev[1].data_ptr(), q.H, q.W, q.pitch)
    refused(hip, hip.set_reduction(R(0, q.fW, q.fH)), "factor = 0")
    refused(hip, hip.set_reduction(q.reduction()), "in flight")
    _, _, st = hip.wait_status()
    orc.track(*q.small[nxt[0]])
    nxt[0] += 1
    assert st == orc.status == 2
    # accepted now; with one more trailing column and row as well
    assert hip.set_reduction(R(2, q.fW + 1, q.fH + 1)) == 0, hip.last_error()
    assert hip.set_reduction(q.reduction()) == 0, hip.last_error()
    next_frame(large=True)

    # per frame, on the reduced handle
    def frame_refused(call, *words):
        before = hip.host_stats()["enqueued"]
        call()
        assert hip.host_stats()["enqueued"] == before and hip.last_error() != "", hip.last_error()
        for w in words:
            assert w in hip.last_error(), (w, hip.last_error())
        said.append(hip.last_error())
    i = nxt[0]
    frame_refused(lambda: hip.track(*q.small[i]), "size")                                                    # the tracker's own size
    frame_refused(lambda: hip.track(q.large[i][0][:-1], q.large[i][1][:-1]), "size")
    frame_refused(lambda: hip.track_async(*q.small[i]), "size")
    big = device_plane(q.large[i][0], 1)
    frame_refused(lambda: hip.track_device_async(big[1], big[1], q.H, q.W, big[2]), "size")
    frame_refused(lambda: hip.track_device_async(big[1], big[1], q.fH, q.fW, q.fW - 1), "pitch")
    cl = np.array([[100.0, 50.0]])
    frame_refused(lambda: hip.track_with_external_corners(*q.large[i], cl, cl), "reduction in force")
    rect = hip_lib.Rectifier(np.array([[q.prm.fx, 0, q.prm.cx], [0, q.prm.fy, q.prm.cy], [0, 0, 1]]), np.zeros(5), np.eye(3),
                             np.array([[q.prm.fx, 0, q.prm.cx], [0, q.prm.fy, q.prm.cy], [0, 0, 1]]), q.W, q.H)
    refused(hip, hip.set_rectifiers(rect, rect), "reduction in force")
    refused(hip, hip.set_rectifiers(None, None), "reduction in force")
    next_frame(large=True)
    assert hip.reduction().factor == 2

    # RGB-D on a reduced sequence without a depth camera
    t = RU.large_world("tum", 3, (640, 480), 2)
    rg = reduced_system(hip_lib, t)
    before = rg.host_stats()["enqueued"]
    rg.track(t.large[0], np.ones((t.fH, t.fW), np.float32))
    assert "no depth camera" in rg.last_error() and rg.last_error().endswith("(nothing was enqueued)") and rg.host_stats()["enqueued"] == before, rg.last_error()
    assert rg.track_async(t.large[0], np.ones((t.H, t.W), np.float32)) == -1 and "no depth camera" in rg.last_error()
    g = device_plane(t.large[0], 1)
    d = torch.ones((t.fH, t.fW), dtype=torch.float32, device="cuda")
    assert rg.track_rgbd_device_async(g[1], d.data_ptr(), t.fH, t.fW, g[2], 4 * t.fW) == -1 and "no depth camera" in rg.last_error()
    assert rg.host_stats()["enqueued"] == before


def C_byref(x):
    import ctypes
    return ctypes.byref(x)


def test_a_set_is_a_use_of_an_lvt_create_handle(hip_lib, oracle_lib, tmp_path):
    q = kitti2()
    q.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    first = hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1)
    assert first.set_reduction(q.reduction()) == 0, first.last_error()
    second = hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1)
    assert first.ordering() != "pooled"
    first.track(*q.large[0])
    assert first.last_error() == "", first.last_error()
    second.close(); first.close()
