"""STREAM ORDER: lvt_amd_set_stream and the stream arguments of the stage entry points (include/lvt_amd_ext.h, "a CALLER'S stream").

Part 1 -- a tracker on a caller's stream.  A delayed producer (stream_util.py: 2 - 10 ms of torch work, then the copies) writes every frame into one of a few
device planes ON the stream the handle was given, and the frame call follows without any host synchronisation.  The plane still holds an older frame of the
same sequence -- a valid image, so a tracker that reads early computes other poses, it never faults.  The reference of every case is a second handle of this
library on its PRIVATE stream, fed the same planes with every write synchronised on the host before the call; once per world that reference run is itself
held to the oracle with parity_util.diff_frame (the route test_gpu_parity.py holds), so the comparison is anchored.  Compared bit for bit: pose bytes and state
of EVERY frame of every case; counters, features of both eyes and the map behind every frame of the synchronous routes and behind the last frame where frames
stay in flight (the getters drain the pipeline: read in between they would end the overlap the case is about).

The planes are the tracker's until their frame has been collected (item 3 of the contract), so a case with d frames in flight rotates d planes: the plane
frame i is produced into was last used by frame i - d, which the host has collected.  The synchronous route uses two.

Part 2 -- the stage entry points on a busy non-default stream: producer -> call -> copy of the result, one stream.synchronize() at the end, compared exactly with
the references the stage tests already use."""
import numpy as np
import pytest

import clahe_util as CL
import colour_util as CU
import depth_reg_util as D
import stream_util as SU
from case_tables import HAMMING_FAMILIES, HAMMING_GEOMETRY, hamming_instance_problem
from hamming_util import hamming_ref, mismatches
from parity_util import make_case, diff_frame, pose_errors, POSE_TOL
from rgbd_util import RSeq, SCALE
from test_gpu_depth_registration import small_prm, scaled_camera, synth_depth, bits
from test_gpu_raw_frames import get_case

pytestmark = pytest.mark.gpu

N_STEREO, N_RGBD = 8, 6
TILES, CLIP = (8, 4), 3.0


# ---- frames in HBM, the planes they are produced into, and the call that hands a plane set to a handle ------------------------------------------------
class StereoFeed:
    """stereo frames (gray (H, W), colour (H, W, bpp) or raw) held tightly packed in HBM, and `nplanes` pitched plane pairs; plane pair k starts out holding
    frame n - 1 - k: what a reader that does not wait for the producer finds is an image of the sequence, only the wrong one"""

    def __init__(self, frames, W, H, bpp=1, pitch=None, nplanes=3, pad=0):
        import torch
        self.W, self.H, self.n, self.nplanes, self.rb = W, H, len(frames), nplanes, W * bpp
        self.pitch = pitch or (self.rb + 63) // 64 * 64
        self.src = torch.from_numpy(np.stack([np.stack([np.ascontiguousarray(e).reshape(H, self.rb) for e in pair]) for pair in frames])).cuda()
        self.planes = torch.full((nplanes, 2, H, self.pitch), pad, dtype=torch.uint8, device="cuda")
        for k in range(nplanes):
            self.planes[k, :, :, :self.rb] = self.src[self.n - 1 - k]
        torch.cuda.synchronize()

    def copies(self, k, i):
        return [(self.planes[k, e, :, :self.rb], self.src[i, e]) for e in (0, 1)]

    def ptrs(self, k):
        return self.planes[k, 0].data_ptr(), self.planes[k, 1].data_ptr()

    def track(self, h, k):
        return h.track_device(*self.ptrs(k), self.H, self.W, self.pitch)

    def track_async(self, h, k):
        h.track_device_async(*self.ptrs(k), self.H, self.W, self.pitch)


class RgbdFeed:
    """the same for RGB-D frames: a gray plane and a 16-bit depth plane whose rows are padded by 6 elements (rgbd_util's layout)"""

    def __init__(self, q, nplanes=3):
        import torch
        self.W, self.H, self.n, self.nplanes = q.W, q.H, q.n, nplanes
        self.gpitch, self.dcols = (q.W + 63) // 64 * 64, q.W + 6
        self.src_g = torch.from_numpy(np.stack(q.gray)).cuda()
        self.src_d = torch.from_numpy(np.stack(q.u16).view(np.int16)).cuda()
        self.pg = torch.zeros((nplanes, q.H, self.gpitch), dtype=torch.uint8, device="cuda")
        self.pd = torch.full((nplanes, q.H, self.dcols), 15000, dtype=torch.int16, device="cuda")
        for k in range(nplanes):
            self.pg[k, :, :q.W] = self.src_g[q.n - 1 - k]
            self.pd[k, :, :q.W] = self.src_d[q.n - 1 - k]
        torch.cuda.synchronize()

    def copies(self, k, i):
        return [(self.pg[k, :, :self.W], self.src_g[i]), (self.pd[k, :, :self.W], self.src_d[i])]

    def _args(self, k, hip_lib):
        return (self.pg[k].data_ptr(), self.pd[k].data_ptr(), self.H, self.W, self.gpitch, 2 * self.dcols, hip_lib.DEPTH_U16, float(SCALE))

    def track(self, h, k):
        import lvt_amd
        got = h.track_rgbd_device(*self._args(k, lvt_amd))
        assert got is not None, h.last_error()
        return got

    def track_async(self, h, k):
        import lvt_amd
        assert h.track_rgbd_device_async(*self._args(k, lvt_amd)) == 0, h.last_error()


# every handle of a test is closed behind it, passed or failed: a handle created beside a live one orders its streams with events, and a failed test's
# traceback would keep its handles alive for the tests behind it
_OPEN = []


def opened(h):
    if h not in _OPEN:
        _OPEN.append(h)
    return h


@pytest.fixture(autouse=True)
def close_handles():
    yield
    while _OPEN:
        _OPEN.pop().close()


# ---- records ---------------------------------------------------------------------------------------------------------------------------------------
def full_record(h, R, t):
    return dict(R=np.asarray(R).tobytes(), t=np.asarray(t).tobytes(), state=h.get_state(), qp=h.pose(), counts=h.counts(), f0=h.features(0), f1=h.features(1), map=h.map())


def same_pose(got, ref, what):
    """(R bytes, t bytes, state) of a collected frame against the reference's record of it"""
    assert got[0] == ref["R"] and got[1] == ref["t"], \
        f"{what}: pose differs: t {np.frombuffer(got[1])} reference {np.frombuffer(ref['t'])}"
    assert got[2] == ref["state"], f"{what}: state {got[2]} reference {ref['state']}"


def same_full(got, ref, what):
    same_pose((got["R"], got["t"], got["state"]), ref, what)
    bad = {k: (got["counts"].get(k), v) for k, v in ref["counts"].items() if got["counts"].get(k) != v}
    assert not bad, f"{what}: counters (caller's stream, reference) {bad}"
    for key, names in (("qp", ("q", "p")), ("f0", ("xy", "resp", "desc")), ("f1", ("xy", "resp", "desc")), ("map", ("xyz", "counter", "age", "desc"))):
        for a, b, name in zip(got[key], ref[key], names):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {key}.{name} differs"


def reference_run(feed, n, make, orc=None, orc_track=None, first=0):
    """frames first .. first + n - 1 through a handle on its PRIVATE stream: every write is synchronised on the host before the call.  With an oracle: every
    frame is held to it.  Returns (the full record of every frame, the handle's ordering)"""
    import torch
    h, s, out = opened(make()), torch.cuda.Stream(), []
    for j in range(n):
        i, k = first + j, j % feed.nplanes
        SU.produce(s, feed.copies(k, i), delayed=False)
        torch.cuda.synchronize()
        R, t = feed.track(h, k)
        if orc is not None:
            Ro, to = orc_track(i)
            msgs = diff_frame(h, orc)
            e_t, e_R = pose_errors(R, t, np.array(Ro), np.array(to))
            assert not msgs, f"reference run, frame {i}: {msgs[:6]}"
            assert e_t <= POSE_TOL and e_R <= POSE_TOL and orc.status == 2, f"reference run, frame {i}: e_t {e_t:.2e} e_R {e_R:.2e} oracle state {orc.status}"
        out.append(full_record(h, R, t))
    assert h.last_error() == "", h.last_error()
    ordering = h.ordering()
    h.close()
    return out, ordering


def drive(h, feed, n, stream, depth, first=0, delayed=True, collect_all=True):
    """frames first .. first + n - 1 through h, each written by the (delayed) producer on `stream` with NO host synchronisation in front of the call.
    depth 0: the synchronous call, the full record of every frame.  depth d > 0: the asynchronous call with d frames in flight, (R, t, state) of every
    frame collected; collect_all False leaves the last d - 1 in flight.  Returns (records, calls that returned while their producer was still running)"""
    out, inflight, raced = [], 0, 0
    assert depth == 0 or depth <= feed.nplanes
    for j in range(n):
        i, k = first + j, j % feed.nplanes
        SU.produce(stream, feed.copies(k, i), delayed)
        if depth == 0:
            R, t = feed.track(h, k)
            out.append(full_record(h, R, t))
            continue
        marker = SU.pending_marker(stream)
        feed.track_async(h, k)
        raced += 0 if marker.query() else 1
        inflight += 1
        if inflight >= depth:
            R, t, st = h.wait_status(); inflight -= 1
            out.append((R.tobytes(), t.tobytes(), st))
    while collect_all and inflight:
        R, t, st = h.wait_status(); inflight -= 1
        out.append((R.tobytes(), t.tobytes(), st))
    return out, raced


def check_in_flight(h, got, ref, what):
    """every collected frame's pose and state, then -- drained -- the last frame's whole record"""
    assert len(got) == len(ref)
    for i, g in enumerate(got):
        same_pose(g, ref[i], f"{what}, frame {i}")
    assert h.last_error() == "", h.last_error()
    R, t = np.frombuffer(got[-1][0]), np.frombuffer(got[-1][1])
    same_full(full_record(h, R, t), ref[-1], f"{what}, behind the last frame")


# ---- the worlds, rendered once; their reference runs, made once ---------------------------------------------------------------------------------------
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def kitti_frames(n=N_STEREO + 2):
    world, prm, _ = make_case("kitti", 71, size=(621, 187))
    return world, prm, cached(("kitti frames", n), lambda: [tuple(np.ascontiguousarray(x) for x in world.render_stereo(i)) for i in range(n)])


def stereo_case(hip_lib, oracle_lib):
    """(feed, prm, reference records, ordering) of the stereo world; the reference run is held to the oracle"""
    def make():
        world, prm, frames = kitti_frames()
        feed = StereoFeed(frames, world.W, world.H)
        orc = oracle_lib.Oracle(prm, 1)
        ref, ordering = reference_run(feed, N_STEREO, lambda: hip_lib.LvtSystem.create(prm, 1), orc, lambda i: orc.track(*frames[i]))
        assert [r["state"] for r in ref] == [2] * N_STEREO
        return feed, prm, ref, ordering
    return cached("stereo", make)


def rgbd_case(hip_lib, oracle_lib):
    def make():
        q = RSeq(86, {}, (320, 240), N_RGBD, device=False)
        feed = RgbdFeed(q)
        orc = oracle_lib.Oracle(q.prm, 2)
        ref, ordering = reference_run(feed, N_RGBD, lambda: hip_lib.LvtSystem.create(q.prm, 2), orc, lambda i: orc.track_rgbd(q.gray[i], q.f32[i]))
        assert [r["state"] for r in ref] == [2] * N_RGBD
        return feed, q.prm, ref, ordering
    return cached("rgbd", make)


def on_stream(h, stream):
    opened(h)
    h.set_stream(stream.cuda_stream)
    assert h.last_error() == "", h.last_error()
    return h


# ---- 1. ordering behind the caller's stream ---------------------------------------------------------------------------------------------------------
def test_track_device_async_three_in_flight(hip_lib, oracle_lib):
    """lvt_amd_track_device_async, three frames in flight, every frame written by the delayed producer on the handle's stream"""
    import torch
    feed, prm, ref, ordering = stereo_case(hip_lib, oracle_lib)
    s = torch.cuda.Stream()
    h = on_stream(hip_lib.LvtSystem.create(prm, 1), s)
    got, raced = drive(h, feed, N_STEREO, s, 3)
    print(f"{raced} of {N_STEREO} calls returned while their producer was still running; ordering {h.ordering()}")
    assert raced > 0, "no call returned ahead of its producer: the case did not exercise the order it is about"
    assert h.ordering() == ordering
    check_in_flight(h, got, ref, "track_device_async")
    h.close()


def test_track_device_synchronous(hip_lib, oracle_lib):
    """lvt_amd_track_device: the whole record of every frame"""
    import torch
    feed, prm, ref, ordering = stereo_case(hip_lib, oracle_lib)
    s = torch.cuda.Stream()
    h = on_stream(hip_lib.LvtSystem.create(prm, 1), s)
    got, _ = drive(h, feed, N_STEREO, s, 0)
    for i in range(N_STEREO):
        same_full(got[i], ref[i], f"track_device, frame {i}")
    assert h.last_error() == "" and h.ordering() == ordering, h.last_error()
    h.close()


@pytest.mark.parametrize("depth", [3, 0], ids=["async_three_in_flight", "synchronous"])
def test_rgbd_gray_and_depth_from_the_producer(hip_lib, oracle_lib, depth):
    """lvt_amd_track_rgbd_device[_async]: the gray plane and the 16-bit depth plane are both written by the delayed producer"""
    import torch
    feed, prm, ref, ordering = rgbd_case(hip_lib, oracle_lib)
    s = torch.cuda.Stream()
    h = on_stream(hip_lib.LvtSystem.create(prm, 2), s)
    got, _ = drive(h, feed, N_RGBD, s, depth)
    if depth:
        check_in_flight(h, got, ref, "track_rgbd_device_async")
    else:
        for i in range(N_RGBD):
            same_full(got[i], ref[i], f"track_rgbd_device, frame {i}")
    assert h.last_error() == "" and h.ordering() == ordering, h.last_error()
    h.close()


def _colour_equalised(hip_lib, prm):
    h = hip_lib.LvtSystem.create(prm, 1)
    assert h.set_pixel_format(hip_lib.PIX_RGB8) == 0 and h.set_equalisation(tiles=TILES, clip_limit=CLIP) == 0, h.last_error()
    return h


def _raw(hip_lib, c, keep):
    h = hip_lib.LvtSystem.create(c.prm, 1)
    rl, rr = c.rectifiers(hip_lib)
    keep.append((rl, rr))
    assert h.set_rectifiers(rl, rr) == 0, h.last_error()
    return h


@pytest.mark.parametrize("kind", ["rgb8_equalised", "raw"])
def test_frame_properties_are_the_first_readers(hip_lib, oracle_lib, kind):
    """a colour (RGB8) and equalised handle, and a raw handle with case A's pincushion rectifier pair: k_gray_frames / k_rectify_frames at the head of the
    feature stage are the first kernels to read the caller's planes.  Three in flight and synchronous; the reference is the same kind of handle on its private
    stream"""
    import torch
    world, prm, frames = kitti_frames()
    keep = []
    if kind == "raw":
        c = get_case("A")
        assert (c.W, c.H) == (world.W, world.H)
        feed = cached("raw feed", lambda: StereoFeed(c.raw[:N_STEREO], c.W, c.H, pitch=640, pad=255))
        make = lambda: _raw(hip_lib, c, keep)   # noqa: E731
    else:
        col = cached("colour frames", lambda: [tuple(CU.colourise(g, CU.RGB8, 71, i, e) for e, g in enumerate(pair)) for i, pair in enumerate(frames[:N_STEREO])])
        feed = cached("colour feed", lambda: StereoFeed(col, world.W, world.H, bpp=3, pad=255))
        make = lambda: _colour_equalised(hip_lib, prm)   # noqa: E731
    ref, ordering = cached(("props reference", kind), lambda: reference_run(feed, N_STEREO, make))
    assert [r["state"] for r in ref] == [2] * N_STEREO, "the reference is not TRACKING throughout: an early LOST would hide a difference"
    for depth in (3, 0):
        s = torch.cuda.Stream()
        h = on_stream(make(), s)
        got, _ = drive(h, feed, N_STEREO, s, depth)
        if depth:
            check_in_flight(h, got, ref, f"{kind}, three in flight")
        else:
            for i in range(N_STEREO):
                same_full(got[i], ref[i], f"{kind}, synchronous, frame {i}")
        assert h.last_error() == "" and h.ordering() == ordering, h.last_error()
        h.close()


# ---- batches ------------------------------------------------------------------------------------------------------------------------------------------
def batch_drive(batch, feeds, offsets, steps, stream, depth, delayed, sync_before, mixed):
    """`steps` lock-step steps, sequence s on frame step + offsets[s]: ONE producer writes every sequence's planes.  [(R, t, state) bytes per step], and every
    sequence's counters behind the last step"""
    import torch
    got, inflight = [], 0

    def collect():
        R, t, st = batch.wait()
        got.append((R.tobytes(), t.tobytes(), st.tobytes()))
    for i in range(steps):
        k = i % feeds[0].nplanes
        SU.produce(stream, [c for f, o in zip(feeds, offsets) for c in f.copies(k, i + o)], delayed)
        if sync_before:
            torch.cuda.synchronize()
        lp, rp = [f.ptrs(k)[0] for f in feeds], [f.ptrs(k)[1] for f in feeds]
        if mixed:
            assert batch.track_device_async_mixed(lp, rp, [f.H for f in feeds], [f.W for f in feeds], [f.pitch for f in feeds]) == 0, batch.last_error()
        else:
            batch.track_device_async(lp, rp, feeds[0].H, feeds[0].W, feeds[0].pitch)
        inflight += 1
        if inflight >= depth:
            collect(); inflight -= 1
    while inflight:
        collect(); inflight -= 1
    assert batch.last_error() == "", batch.last_error()
    return got, [batch.counts(s) for s in range(len(feeds))]


def same_batch(got, ref, B, what):
    assert len(got[0]) == len(ref[0])
    for k, (g, r) in enumerate(zip(got[0], ref[0])):
        for name, a, b, dt in (("R", g[0], r[0], np.float64), ("t", g[1], r[1], np.float64), ("state", g[2], r[2], np.int32)):
            if a != b:
                x, y = np.frombuffer(a, dt).reshape(B, -1), np.frombuffer(b, dt).reshape(B, -1)
                s = int(np.argwhere((x != y).any(axis=1))[0][0])
                raise AssertionError(f"{what}: step {k}, sequence {s}: {name} {x[s]} reference {y[s]}")
    for s in range(B):
        bad = {k: (got[1][s].get(k), v) for k, v in ref[1][s].items() if got[1][s].get(k) != v}
        assert not bad, f"{what}: sequence {s}: counters behind the last step (caller's stream, reference) {bad}"


def uniform_batch_case(hip_lib, oracle_lib):
    """three sequences of the stereo world, one frame apart; the reference batch on its private streams, whose sequence 0 is the single handle's reference"""
    def make():
        import torch
        world, prm, frames = kitti_frames()
        feeds = [StereoFeed(frames, world.W, world.H) for _ in range(3)]
        batch = opened(hip_lib.LvtBatch(prm, 3))
        ref = batch_drive(batch, feeds, (0, 1, 2), N_STEREO, torch.cuda.Stream(), 3, False, True, False)
        batch.close()
        single = stereo_case(hip_lib, oracle_lib)[2]
        for k in range(N_STEREO):
            assert ref[0][k][0][:72] == single[k]["R"] and ref[0][k][1][:24] == single[k]["t"], f"the reference batch's sequence 0 leaves the single handle at step {k}"
        return feeds, prm, ref
    return cached("uniform batch", make)


def mixed_batch_case(hip_lib):
    def make():
        import torch
        world, prm, frames = kitti_frames()
        w2, prm2, _ = make_case("kitti", 32, size=(620, 188))
        frames2 = [tuple(np.ascontiguousarray(x) for x in w2.render_stereo(i)) for i in range(N_STEREO)]
        feeds = [StereoFeed(frames, world.W, world.H), StereoFeed(frames2, w2.W, w2.H)]
        batch = opened(hip_lib.LvtBatch([prm, prm2]))
        ref = batch_drive(batch, feeds, (0, 0), N_STEREO, torch.cuda.Stream(), 3, False, True, True)
        batch.close()
        assert np.frombuffer(ref[0][-1][2], np.int32).tolist() == [2, 2]
        return feeds, [prm, prm2], ref
    return cached("mixed batch", make)


def test_uniform_batch_of_three(hip_lib, oracle_lib):
    """lvt_amd_batch_track_device_async on a caller's stream, three steps in flight: a batch of 3 has a CU-masked feature stream, which waits like any other"""
    import torch
    feeds, prm, ref = uniform_batch_case(hip_lib, oracle_lib)
    s = torch.cuda.Stream()
    batch = on_stream(hip_lib.LvtBatch(prm, 3), s)
    got = batch_drive(batch, feeds, (0, 1, 2), N_STEREO, s, 3, True, False, False)
    same_batch(got, ref, 3, "uniform batch")
    batch.close()


def test_mixed_batch_of_two(hip_lib, oracle_lib):
    """lvt_amd_batch_track_device_async_mixed: 621 x 187 beside 620 x 188"""
    import torch
    feeds, prms, ref = mixed_batch_case(hip_lib)
    s = torch.cuda.Stream()
    batch = on_stream(hip_lib.LvtBatch(prms), s)
    got = batch_drive(batch, feeds, (0, 0), N_STEREO, s, 3, True, False, True)
    same_batch(got, ref, 2, "mixed batch")
    batch.close()


# ---- the NULL stream ----------------------------------------------------------------------------------------------------------------------------------
def test_null_stream_single_handle(hip_lib, oracle_lib):
    """lvt_amd_set_stream(h, NULL) -- what the header's example passes on torch's default stream: the producer runs on the legacy default stream"""
    import torch
    feed, prm, ref, ordering = stereo_case(hip_lib, oracle_lib)
    s = torch.cuda.default_stream()
    assert s.cuda_stream == 0
    for depth in (3, 0):
        h = on_stream(hip_lib.LvtSystem.create(prm, 1), s)
        got, raced = drive(h, feed, N_STEREO, s, depth)
        if depth:
            print(f"{raced} of {N_STEREO} calls returned while their producer was still running")
            check_in_flight(h, got, ref, "NULL stream, three in flight")
        else:
            for i in range(N_STEREO):
                same_full(got[i], ref[i], f"NULL stream, synchronous, frame {i}")
        assert h.last_error() == "" and h.ordering() == ordering, h.last_error()
        h.close()
    torch.cuda.synchronize()


def test_null_stream_batch(hip_lib, oracle_lib):
    """a batch accepts the NULL stream too: its CU-masked feature stream synchronises with the legacy default stream, which adds waits for earlier work only
    ("A caller's stream") -- no gate times out (last_error stays empty) and the records are the reference batch's"""
    import torch
    feeds, prm, ref = uniform_batch_case(hip_lib, oracle_lib)
    s = torch.cuda.default_stream()
    batch = on_stream(hip_lib.LvtBatch(prm, 3), s)
    got = batch_drive(batch, feeds, (0, 1, 2), N_STEREO, s, 3, True, False, False)
    same_batch(got, ref, 3, "batch on the NULL stream")
    batch.close()
    torch.cuda.synchronize()


# ---- 2. the other promises ------------------------------------------------------------------------------------------------------------------------------
def test_changing_the_stream_between_frames(hip_lib, oracle_lib):
    """private stream (3 frames, 2 left in flight) -> s1 (2 frames, left in flight) -> s2 (2 frames, synchronous) -> close: set_stream collects what is in
    flight (host stats), the records follow the reference throughout, and both streams outlive the handle"""
    import torch
    feed, prm, ref, ordering = stereo_case(hip_lib, oracle_lib)
    s0, s1, s2 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    h = opened(hip_lib.LvtSystem.create(prm, 1))
    got = []
    for i in range(3):                                    # (a private stream is ordered behind nothing of the caller's: host-synchronised writes)
        SU.produce(s0, feed.copies(i % 3, i), delayed=False)
        torch.cuda.synchronize()
        feed.track_async(h, i % 3)
    R, t, st = h.wait_status()
    same_pose((R.tobytes(), t.tobytes(), st), ref[0], "private stream, frame 0")
    hs = h.host_stats()
    assert (hs["enqueued"], hs["collected"]) == (3, 1), hs
    on_stream(h, s1)
    hs = h.host_stats()
    assert (hs["enqueued"], hs["collected"]) == (3, 3), f"set_stream left frames in flight: {hs}"
    same_full(full_record(h, np.frombuffer(ref[2]["R"]), np.frombuffer(ref[2]["t"])), dict(ref[2]), "behind set_stream(s1), frame 2")
    got, _ = drive(h, feed, 2, s1, 3, first=3, collect_all=False)      # frames 3, 4 on s1: nothing collected yet
    assert got == [] and h.host_stats()["collected"] == 3
    on_stream(h, s2)
    hs = h.host_stats()
    assert (hs["enqueued"], hs["collected"]) == (5, 5), f"set_stream left frames in flight: {hs}"
    same_full(full_record(h, np.frombuffer(ref[4]["R"]), np.frombuffer(ref[4]["t"])), dict(ref[4]), "behind set_stream(s2), frame 4")
    got, _ = drive(h, feed, 2, s2, 0, first=5)
    for j in range(2):
        same_full(got[j], ref[5 + j], f"on s2, frame {5 + j}")
    assert h.last_error() == "" and h.ordering() == ordering, h.last_error()
    h.close()
    for s in (s1, s2):                                    # destroying the handle never destroys a caller's stream
        with torch.cuda.stream(s):
            x = torch.arange(1000, device="cuda").sum()
        s.synchronize()
        assert int(x) == 499500


def test_a_set_is_a_use_of_an_lvt_create_handle(hip_lib, oracle_lib, tmp_path):
    """lvt_create, set_stream, a second lvt_create with the same parameters: the first handle keeps its own chain -- on the caller's stream, ordered behind it"""
    import torch
    feed, prm, _, _ = stereo_case(hip_lib, oracle_lib)
    cfg = str(tmp_path / "cfg.yaml")
    prm.write_yaml(cfg)
    ref, ordering = reference_run(feed, N_STEREO, lambda: hip_lib.LvtSystem.create_from_file(cfg, 1))   # (the parameters as the file carries them)
    s = torch.cuda.Stream()
    first = on_stream(hip_lib.LvtSystem.create_from_file(cfg, 1), s)
    second = opened(hip_lib.LvtSystem.create_from_file(cfg, 1))
    assert first.ordering() != "pooled"
    got, _ = drive(first, feed, N_STEREO, s, 3)
    check_in_flight(first, got, ref, "lvt_create handle on a caller's stream")
    second.close(); first.close()


# (last of the trackers: a pool that stays alive moves the handles created beside it to event ordering)
def test_a_pooled_seat_ignores_the_call(hip_lib, oracle_lib):
    """a seat runs on its pool's streams: set_stream changes nothing, the seat goes on tracking -- fed host-synchronised planes -- and equals the reference"""
    import torch
    feed, prm, ref, _ = stereo_case(hip_lib, oracle_lib)
    s = torch.cuda.Stream()
    seat = opened(hip_lib.LvtSystem.create(prm, 1, pooled=True))
    assert seat.ordering() == "pooled"
    seat.set_stream(s.cuda_stream)
    assert seat.ordering() == "pooled" and seat.last_error() == ""
    for i in range(N_STEREO):
        SU.produce(s, feed.copies(i % 3, i), delayed=False)
        torch.cuda.synchronize()
        R, t = feed.track(seat, i % 3)
        same_pose((R.tobytes(), t.tobytes(), seat.get_state()), ref[i], f"pooled seat, frame {i}")
        assert seat.counts() == ref[i]["counts"], f"pooled seat, frame {i}"
    assert seat.last_error() == "", seat.last_error()
    seat.close()


# ---- 3. the stage entry points on a busy stream ------------------------------------------------------------------------------------------------------
GUARD = 0xA5


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()       # (a copy: the case tables hand out read-only arrays)


def test_rectify_device_on_a_busy_stream(hip_lib, oracle_lib):
    """lvt_amd_rectify_device against O.remap_bilinear with the oracle's maps, byte for byte: case A (pincushion), the source at pitch 629 with 255 in its
    padding, destination pitches 624 / 640 / 1024 with a guard row behind the plane; the refused arguments write nothing"""
    import torch
    c = get_case("A")
    W, H, sp = c.W, c.H, 629
    m1, m2 = c.maps[0]
    outside = float(np.mean((m1 < 0) | (m1 > W - 1) | (m2 < 0) | (m2 > H - 1)))
    assert outside > 0.05, outside                        # (a condition on the input: the border branches run)
    rect = c.rectifiers(hip_lib)[0]
    raw, want = _dev(c.raw[0][0]), c.rect[0][0]
    s = torch.cuda.Stream()
    for dp in (624, 640, 1024):
        src = torch.full((H, sp), 255, dtype=torch.uint8, device="cuda")
        src[:, :W] = _dev(c.raw[1][0])                    # (what an early reader would remap: another frame)
        dst = torch.full((H + 1, dp), GUARD, dtype=torch.uint8, device="cuda")
        res = torch.zeros_like(dst)
        torch.cuda.synchronize()
        SU.produce(s, [(src[:, :W], raw)])
        assert rect.rectify_device(src.data_ptr(), sp, dst.data_ptr(), dp, s.cuda_stream) == 0
        with torch.cuda.stream(s):
            res.copy_(dst, non_blocking=True)
        s.synchronize()
        got = res.cpu().numpy()
        bad = np.argwhere(got[:H, :W] != want)
        assert len(bad) == 0, f"dst_pitch {dp}: {len(bad)} pixels differ, first at {tuple(bad[0])}: hip {got[tuple(bad[0])]} oracle {want[tuple(bad[0])]}"
        assert not got[:H, W:].any(), f"dst_pitch {dp}: the padding columns are not zero"
        assert (got[H] == GUARD).all(), f"dst_pitch {dp}: bytes behind dst_pitch * h were written"
    dst = torch.full((H + 1, 640), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for args in ((src.data_ptr(), sp, dst.data_ptr(), 622), (src.data_ptr(), W - 1, dst.data_ptr(), 640), (src.data_ptr(), sp, dst.data_ptr(), 620),
                 (0, sp, dst.data_ptr(), 640), (src.data_ptr(), sp, 0, 640)):
        assert rect.rectify_device(*args, s.cuda_stream) == -1, args[1::2]
    s.synchronize()
    assert bool((dst == GUARD).all()), "a refused call wrote"


def test_equalise_device_on_a_busy_stream(hip_lib):
    """lvt_amd_equalise_device against clahe_util: 64 x 64, 8 x 8 tiles"""
    import torch
    W, H, tiles, clip = 64, 64, (8, 8), 3.0
    img = np.random.default_rng(64064).integers(0, 256, (H, W), dtype=np.uint8)
    want = CL.clahe(img, tiles, clip)
    sp, dp = W + 5, W + 8
    src = torch.full((H, sp), 255, dtype=torch.uint8, device="cuda")
    src[:, :W] = _dev(img.T.copy())                       # (what an early reader would equalise)
    dst = torch.full((H + 1, dp), GUARD, dtype=torch.uint8, device="cuda")
    res, s = torch.zeros_like(dst), torch.cuda.Stream()
    torch.cuda.synchronize()
    SU.produce(s, [(src[:, :W], _dev(img))])
    assert hip_lib.equalise_device(hip_lib.Equalisation(tiles, clip), src.data_ptr(), sp, W, H, dst.data_ptr(), dp, s.cuda_stream) == 0
    with torch.cuda.stream(s):
        res.copy_(dst, non_blocking=True)
    s.synchronize()
    got = res.cpu().numpy()
    assert np.array_equal(got[:H, :W], want) and not got[:H, W:].any() and (got[H] == GUARD).all()


def test_register_depth_device_on_a_busy_stream(hip_lib):
    """lvt_amd_register_depth_device against depth_reg_util: 80 x 60 -> 160 x 120, every word's bits"""
    import torch
    prm = small_prm(hip_lib, 160, 120)
    cam = scaled_camera(prm, 80, 60, t=(0.05, 0, 0))
    d = synth_depth(80, 60, 2)
    want = D.register(cam, prm, d, None, pitch=160)
    src = _dev(np.ascontiguousarray(d[::-1]))             # (what an early reader would register)
    out = torch.full((120, 160), -3.0, dtype=torch.float32, device="cuda")
    res, s = torch.zeros_like(out), torch.cuda.Stream()
    torch.cuda.synchronize()
    SU.produce(s, [(src, _dev(d))])
    assert hip_lib.register_depth_device(cam, prm, src.data_ptr(), 4 * 80, hip_lib.DEPTH_F32, 0.0, out.data_ptr(), 4 * 160, s.cuda_stream) == 0
    with torch.cuda.stream(s):
        res.copy_(out, non_blocking=True)
    s.synchronize()
    got = res.cpu().numpy()
    bad = np.argwhere(bits(got) != bits(want))
    assert not len(bad), f"{len(bad)} words differ, first (row, column) {tuple(bad[0])}: gpu {got[tuple(bad[0])]!r} numpy {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("fam", ["row", "csr1"])
def test_hamming_match_batched_on_a_busy_stream(hip_lib, fam):
    """lvt_amd_hamming_match_batched against hamming_util, one small case per mode: the query and the train descriptors are written by the producer"""
    import torch
    mode, _, r2 = HAMMING_FAMILIES[fam]
    rows, cols = HAMMING_GEOMETRY
    qd, qxy, td, txy, tf = hamming_instance_problem(fam, 300, 700)
    ref = hamming_ref(qd, qxy, td, txy, tf, r2, mode, rows)
    d_qd, d_td = torch.zeros(qd.shape, dtype=torch.uint8, device="cuda"), torch.zeros(td.shape, dtype=torch.uint8, device="cuda")
    d_qxy, d_txy, d_tf = _dev(qxy), _dev(txy), _dev(tf)
    out = torch.full(qd.shape[:2] + (4,), -77, dtype=torch.int32, device="cuda")
    res, s = torch.zeros_like(out), torch.cuda.Stream()
    torch.cuda.synchronize()
    SU.produce(s, [(d_qd, _dev(qd)), (d_td, _dev(td))])
    us = hip_lib.hamming_match_batched(d_qd, d_qxy, d_td, d_txy, d_tf, float(r2), mode, rows, cols, out, stream=s.cuda_stream)
    assert us > 0
    with torch.cuda.stream(s):
        res.copy_(out, non_blocking=True)
    s.synchronize()
    got = res.cpu().numpy()
    assert np.array_equal(got, ref), f"{fam}: {mismatches(got, ref)}"


def test_rectify_then_equalise_on_one_stream(hip_lib, oracle_lib):
    """producer -> lvt_amd_rectify_device -> lvt_amd_equalise_device on one stream, against the numpy chain of the two references"""
    import torch
    c = get_case("A")
    W, H = c.W, c.H
    want = CL.clahe(c.rect[0][0], TILES, CLIP)
    rect = c.rectifiers(hip_lib)[0]
    src = torch.full((H, 629), 255, dtype=torch.uint8, device="cuda")
    src[:, :W] = _dev(c.raw[1][0])
    mid = torch.full((H, 640), GUARD, dtype=torch.uint8, device="cuda")
    dst = torch.full((H + 1, 624), GUARD, dtype=torch.uint8, device="cuda")
    res, s = torch.zeros_like(dst), torch.cuda.Stream()
    torch.cuda.synchronize()
    SU.produce(s, [(src[:, :W], _dev(c.raw[0][0]))])
    assert rect.rectify_device(src.data_ptr(), 629, mid.data_ptr(), 640, s.cuda_stream) == 0
    assert hip_lib.equalise_device(hip_lib.Equalisation(TILES, CLIP), mid.data_ptr(), 640, W, H, dst.data_ptr(), 624, s.cuda_stream) == 0
    with torch.cuda.stream(s):
        res.copy_(dst, non_blocking=True)
    s.synchronize()
    got = res.cpu().numpy()
    bad = np.argwhere(got[:H, :W] != want)
    assert len(bad) == 0, f"{len(bad)} pixels differ, first at {tuple(bad[0])}: hip {got[tuple(bad[0])]} numpy {want[tuple(bad[0])]}"
    assert not got[:H, W:].any() and (got[H] == GUARD).all()
