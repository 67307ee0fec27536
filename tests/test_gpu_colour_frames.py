"""COLOUR frames: a pixel format per handle / per sequence of a batch (lvt_amd_set_pixel_format / lvt_amd_batch_set_pixel_format), the conversion to gray as the
first launch of the feature stage (k_gray_frames).  No expected value comes from this library: the tests convert with a numpy restatement of the formula
(colour_util.to_gray, held to examples/image_io.h by tests/test_colour_formats.py) and give the ORACLE the converted gray -- O.Oracle.track / track_rgbd /
track_with_external_corners, and O.remap_bilinear with O.init_undistort_rectify_map where rectifiers are attached.

The synthetic worlds render gray; the tests colourise them (colour_util.colourise: independent noise of a different amplitude per channel, random alpha), so
a swapped channel order or a used alpha byte changes most gray pixels.  Every oracle chain is asserted to be TRACKING on every frame before anything is
compared.  Frames that are in flight together (the asynchronous routes) are held to the oracle by state and pose, frame by frame, and by the complete
parity_util.diff_frame behind the last one: the per-stage read-back drains the pipeline, so it cannot be taken between frames that are to stay in flight;
the synchronous routes run diff_frame behind every frame."""
import numpy as np
import pytest

import colour_util as CU
from parity_util import make_case, diff_frame
from test_gpu_raw_frames import get_case as raw_case, close_to, counts_equal, pinned, _run_async as run_async

pytestmark = pytest.mark.gpu

SCALE = np.float32(1) / np.float32(5000)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
class ColourStereo:
    """a stereo world's gray renderings, colourised: the channels of every image (drawn once per world, frame and eye), the gray image the formula makes of
    them, and the oracle's chain on those gray images"""

    def __init__(self, kind, seed, size, n):
        self.world, self.prm, _ = make_case(kind, seed, size=size)
        self.seed, self.W, self.H, self.n = seed, self.world.W, self.world.H, n
        self.pitch = ((self.W + 63) // 64) * 64
        self.chan = [[CU.colour_channels(np.ascontiguousarray(g), seed, i, eye) for eye, g in enumerate(self.world.render_stereo(i))] for i in range(n)]
        self.gray = [tuple(np.ascontiguousarray(CU.gray_of_rgb(*c[:3])) for c in pair) for pair in self.chan]
        self._chains = {}

    def colour(self, i, fmt):
        return tuple(CU.pack(*c, fmt) for c in self.chan[i])

    def oracle(self):
        from oracle import pyoracle as O
        return O.Oracle(self.prm, 1)

    def chain(self, frames=None, images=None):
        """[(R, t, state, counts)] of the oracle over `frames` of the converted gray images (or of `images`), asserted TRACKING throughout"""
        frames = tuple(range(8)) if frames is None else tuple(frames)
        key = (frames, id(images))
        if key not in self._chains:
            orc, out = self.oracle(), []
            for i in frames:
                R, t = orc.track(*(images or self.gray)[i])
                out.append((np.array(R), np.array(t), orc.status, orc.counts()))
            assert [r[2] for r in out] == [2] * len(out), "the oracle is not TRACKING on every frame: an early LOST would hide a difference"
            print("oracle matches:", [r[3]["n_matches"] for r in out])
            self._chains[key] = out
        return self._chains[key]


_SEQS = {}


def stereo_seq(seed, size, n=8):
    key = (seed, size, n)
    if key not in _SEQS:
        _SEQS[key] = ColourStereo("kitti", seed, size, n)
    return _SEQS[key]


class ColourRgbd:
    """the tum world at 322 x 242: colourised gray, 16-bit depth (and the fp32 metres the oracle gets)"""

    def __init__(self, n, seed=0, size=(322, 242)):
        self.world, self.prm, sensor = make_case("tum", seed, 1.0, None, size)
        assert sensor == 2
        self.W, self.H, self.n = self.world.W, self.world.H, n
        self.pitch = ((self.W + 63) // 64) * 64
        self.raw_gray, self.chan, self.gray, self.u16, self.f32 = [], [], [], [], []
        for i in range(n):
            g, d = self.world.render_rgbd(i)
            u = np.clip(np.rint(d.astype(np.float64) * 5000.0), 0, 65535).astype(np.uint16)
            c = CU.colour_channels(np.ascontiguousarray(g), seed, i, 0)
            self.raw_gray.append(np.ascontiguousarray(g)); self.chan.append(c); self.gray.append(np.ascontiguousarray(CU.gray_of_rgb(*c[:3])))
            self.u16.append(u); self.f32.append(u.astype(np.float32) * SCALE)
        self._chains = {}

    def colour(self, i, fmt):
        return CU.pack(*self.chan[i], fmt)

    def chain(self, frames, images=None):
        from oracle import pyoracle as O
        key = (tuple(frames), id(images))
        if key not in self._chains:
            orc, out = O.Oracle(self.prm, 2), []
            for i in frames:
                R, t = orc.track_rgbd((images or self.gray)[i], self.f32[i])
                out.append((np.array(R), np.array(t), orc.status, orc.counts()))
            assert [r[2] for r in out] == [2] * len(out), "the oracle is not TRACKING on every frame"
            self._chains[key] = out
        return self._chains[key]


_RGBD = {}


def rgbd_seq(n=9):
    if n not in _RGBD:
        _RGBD[n] = ColourRgbd(n)
    return _RGBD[n]


def device_colour(img, offset, extra=5, guard=255):
    """one interleaved colour image in HBM at a base `offset` bytes past an aligned address, rows W * bpp + extra bytes apart; every byte before, between
    and behind the rows holds `guard`.  Returns (tensor that owns the memory, device address of the image, pitch)."""
    import torch
    H, row = img.shape[0], img.shape[1] * img.shape[2]
    pitch = row + extra
    buf = np.full(256 + offset + H * pitch + 256, guard, np.uint8)
    np.lib.stride_tricks.as_strided(buf[256 + offset:], shape=(H, row), strides=(pitch, 1))[:] = img.reshape(H, row)
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + 256 + offset, pitch


def device_gray(imgs, W, H, pitch):
    import torch
    t = torch.zeros((len(imgs), H, pitch), dtype=torch.uint8, device="cuda")
    for i, a in enumerate(imgs):
        t[i, :, :W] = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t


def colour_system(hip_lib, prm, fmt, sensor=1):
    hip = hip_lib.LvtSystem.create(prm, sensor)
    assert hip.set_pixel_format(fmt) == 0, hip.last_error()
    assert hip.pixel_format() == fmt
    return hip


def assert_plane(p, want, W, H, pitch, what):
    assert p.shape == (H, pitch) and p.dtype == np.uint8, (what, p.shape)
    bad = np.argwhere(p[:, :W] != want)
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at {tuple(bad[0])}: hip {p[tuple(bad[0])]} numpy {want[tuple(bad[0])]}"
    assert not p[:, W:].any(), f"{what}: the padding columns are not zero"


# ---- 1. the converted plane ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lvt_track", "track_device"])
@pytest.mark.parametrize("W", [620, 621, 622, 623])
@pytest.mark.parametrize("fmt", CU.COLOUR_FORMATS, ids=[CU.NAMES[f] for f in CU.COLOUR_FORMATS])
def test_converted_plane_equals_the_numpy_conversion(hip_lib, oracle_lib, fmt, W, route):
    """after one frame plane(eye, 3)[:, :W] is the numpy conversion byte for byte and the padding columns are zero.  The four widths cover every residue of
    W * 3 mod 4, W mod 4 != 0 and a last destination word that is part image, part padding; the device planes start 1, 2 or 3 bytes past an aligned address
    with a pitch of W * bpp + 5 and 255 in every byte that is not a pixel's: a conversion that used one would show in the plane"""
    q = stereo_seq(71, (W, 187), 1)
    hip = colour_system(hip_lib, q.prm, fmt)
    imgs = q.colour(0, fmt)
    if route == "lvt_track":
        hip.track(*imgs)
    else:
        keep = [device_colour(imgs[eye], 1 + (W + fmt + eye) % 3) for eye in (0, 1)]
        assert {k[1] % 4 for k in keep} <= {1, 2, 3} and keep[0][2] == keep[1][2] == W * CU.BPP[fmt] + 5
        hip.track_device(keep[0][1], keep[1][1], q.H, W, keep[0][2])
    assert hip.last_error() == "", hip.last_error()
    for eye in (0, 1):
        assert_plane(hip.plane(eye, 3), q.gray[0][eye], W, q.H, q.pitch, f"{CU.NAMES[fmt]} W {W} eye {eye}")
    assert hip.plane(0, 2).size == 0


# ---- 2. known answers --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [CU.RGB8, CU.BGRA8, CU.BGR8], ids=["RGB8", "BGRA8", "BGR8"])
def test_known_answers(hip_lib, oracle_lib, fmt):
    """four vertical bands -- pure R, G, B, white -- over a ramp of every gray level as R = G = B: 76 / 150 / 29 / 255 and g, in RGB8 and in BGRA8 (random
    alpha); the RGB8 bytes handed to a BGR8 handle: the R and B bands swap"""
    W, H = 620, 187
    _, prm, _ = make_case("kitti", 71, size=(W, H))
    rgb = np.zeros((H, W, 3), np.uint8)
    for k, px in enumerate([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)]):
        rgb[:94, 155 * k:155 * (k + 1)] = px
    rgb[94:] = (np.arange(W) % 256).astype(np.uint8)[None, :, None]
    alpha = np.random.default_rng(9).integers(0, 256, size=(H, W), dtype=np.uint8)
    img = rgb if fmt == CU.BGR8 else CU.pack(rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2], alpha, fmt)
    hip = colour_system(hip_lib, prm, fmt)
    hip.track(img, img)
    want = np.zeros((H, W), np.uint8)
    bands = [29, 150, 76, 255] if fmt == CU.BGR8 else [76, 150, 29, 255]
    for k, g in enumerate(bands):
        want[:94, 155 * k:155 * (k + 1)] = g
    want[94:] = (np.arange(W) % 256).astype(np.uint8)[None, :]
    assert set(np.unique(want[94:])) == set(range(256))
    for eye in (0, 1):
        assert_plane(hip.plane(eye, 3), want, W, H, 640, f"eye {eye}")


# ---- 3. sequences against the oracle -------------------------------------------------------------------------------------------------------------
def test_colour_sequence_through_lvt_track(hip_lib, oracle_lib):
    """world 71 at 621 x 187, RGB8, 8 frames through lvt_track: the complete frame diff is empty on every frame, poses within POSE_TOL"""
    q = stereo_seq(71, (621, 187))
    ref = q.chain()
    hip, orc = colour_system(hip_lib, q.prm, CU.RGB8), q.oracle()
    for i in range(8):
        Ro, to = orc.track(*q.gray[i])
        R, t = hip.track(*q.colour(i, CU.RGB8))
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, ref[i], f"frame {i}")
        assert orc.status == 2


def check_async(q, hip, got, ref, images=None):
    for i, (R, t, st) in enumerate(got):
        assert st == ref[i][2], f"frame {i}: state {st} oracle {ref[i][2]}"
        close_to(R, t, ref[i], f"frame {i}")
    orc = q.oracle()
    for i in range(len(got)):
        orc.track(*(images or q.gray)[i])
    msgs = diff_frame(hip, orc)
    assert not msgs, msgs[:6]
    counts_equal(hip.counts(), ref[len(got) - 1][3], "last frame")


def one_by_one(hip, submit, orc, track_oracle, ref, n=8):
    """the second pass of an asynchronous route: the same frames through a fresh handle with ONE frame in flight, the complete diff_frame behind every frame"""
    for i in range(n):
        submit(hip, i)
        R, t, st = hip.wait_status()
        track_oracle(orc, i)
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        assert st == orc.status == 2, f"frame {i}: state {st} oracle {orc.status}"
        close_to(R, t, ref[i], f"one by one, frame {i}")


@pytest.mark.parametrize("memory", ["pageable", "page_locked"])
def test_colour_frames_through_track_async(hip_lib, oracle_lib, memory):
    """lvt_amd_track_async on RGB8 host frames, four in flight: the staging and the pull fused into the previous frame's corner-cell launch carry colour bytes;
    then the same frames one by one, every frame through diff_frame"""
    q = stereo_seq(71, (621, 187))
    hip = colour_system(hip_lib, q.prm, CU.RGB8)
    bufs = [tuple(pinned(a) if memory == "page_locked" else a for a in q.colour(i, CU.RGB8)) for i in range(8)]

    def submit(h, i):
        assert h.track_async(*bufs[i]) == 0, h.last_error()
    got = run_async(hip, lambda i: submit(hip, i), 8, 4)
    check_async(q, hip, got, q.chain())
    hs = hip.host_stats()
    assert hs["async_host_frames"] == 8 and (hs["planes_in_place"] if memory == "page_locked" else hs["planes_staged"]) == 16, hs
    assert hs["pulls_carried_by_the_previous_frame"] > 0, hs
    hip.close()
    one_by_one(colour_system(hip_lib, q.prm, CU.RGB8), submit, q.oracle(), lambda orc, i: orc.track(*q.gray[i]), q.chain())


def test_colour_frames_through_track_device_async(hip_lib, oracle_lib):
    """RGB8 planes in HBM at odd addresses with a pitch of W * 3 + 5, three frames in flight, read in place; then one by one, every frame through diff_frame"""
    q = stereo_seq(71, (621, 187))
    hip = colour_system(hip_lib, q.prm, CU.RGB8)
    dev = [[device_colour(img, 1 + (i + eye) % 3) for eye, img in enumerate(q.colour(i, CU.RGB8))] for i in range(8)]

    def submit(h, i):
        h.track_device_async(dev[i][0][1], dev[i][1][1], q.H, q.W, dev[i][0][2])
    got = run_async(hip, lambda i: submit(hip, i), 8, 3)
    assert hip.last_error() == "", hip.last_error()
    check_async(q, hip, got, q.chain())
    hip.close()
    one_by_one(colour_system(hip_lib, q.prm, CU.RGB8), submit, q.oracle(), lambda orc, i: orc.track(*q.gray[i]), q.chain())


def test_colour_frames_with_external_corners(hip_lib, oracle_lib):
    """the same frames as BGRA8 through lvt_track_with_external_corners, the corners taken from the oracle's detector on the converted gray"""
    from oracle import pyoracle as O
    q = stereo_seq(71, (621, 187))
    hip, orc = colour_system(hip_lib, q.prm, CU.BGRA8), q.oracle()
    for i in range(8):
        cl = O.compute_features(q.gray[i][0], q.prm)[0].astype(np.float64)
        cr = O.compute_features(q.gray[i][1], q.prm)[0].astype(np.float64)
        Ro, to = orc.track_with_external_corners(q.gray[i][0], q.gray[i][1], cl, cr)
        R, t = hip.track_with_external_corners(*q.colour(i, CU.BGRA8), cl, cr)
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"


# ---- 4. RGB-D ----------------------------------------------------------------------------------------------------------------------------------
def test_rgbd_colour_host_frames(hip_lib, oracle_lib):
    """BGRA8 colour + 16-bit depth through lvt_amd_track_rgbd16_async, three in flight, against the oracle's track_rgbd on the converted gray; then one
    by one, every frame through diff_frame"""
    from oracle import pyoracle as O
    q = rgbd_seq()
    ref = q.chain(range(8))
    hip = colour_system(hip_lib, q.prm, CU.BGRA8, 2)
    cols = [q.colour(i, CU.BGRA8) for i in range(8)]

    def submit(h, i):
        assert h.track_async(cols[i], q.u16[i], depth_scale=SCALE) == 0, h.last_error()
    got = run_async(hip, lambda i: submit(hip, i), 8, 3)
    for i, (R, t, st) in enumerate(got):
        assert st == ref[i][2], f"frame {i}: state {st}"
        close_to(R, t, ref[i], f"frame {i}")
    orc = O.Oracle(q.prm, 2)
    for i in range(8):
        orc.track_rgbd(q.gray[i], q.f32[i])
    msgs = diff_frame(hip, orc)
    assert not msgs, msgs[:6]
    assert_plane(hip.plane(0, 3), q.gray[7], q.W, q.H, q.pitch, "last frame")
    hip.close()
    one_by_one(colour_system(hip_lib, q.prm, CU.BGRA8, 2), submit, O.Oracle(q.prm, 2), lambda orc, i: orc.track_rgbd(q.gray[i], q.f32[i]), ref)


def test_rgbd_colour_device_frames(hip_lib, oracle_lib):
    """BGRA8 planes in HBM at an odd address with a pitch of W * 4 + 5 through lvt_amd_track_rgbd_device_async, collected one by one: the complete
    frame diff behind every frame"""
    import torch
    from oracle import pyoracle as O
    q = rgbd_seq()
    hip, orc = colour_system(hip_lib, q.prm, CU.BGRA8, 2), O.Oracle(q.prm, 2)
    d16 = torch.from_numpy(np.stack(q.u16[:8]).view(np.int16)).cuda()
    for i in range(8):
        keep = device_colour(q.colour(i, CU.BGRA8), 1 + i % 3)
        assert keep[2] % 4 != 0
        assert hip.track_rgbd_device_async(keep[1], d16[i].data_ptr(), q.H, q.W, keep[2], 2 * q.W, hip_lib.DEPTH_U16, SCALE) == 0, hip.last_error()
        R, t, st = hip.wait_status()
        Ro, to = orc.track_rgbd(q.gray[i], q.f32[i])
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        assert orc.status == 2 == st, f"frame {i}: the oracle is not TRACKING"


# ---- 5. colour and rectifiers together -----------------------------------------------------------------------------------------------------------
class RawColour:
    """case A of test_gpu_raw_frames.py (world 71 at 621 x 187, one pincushion rectifier for both eyes), its raw frames colourised: convert, then remap"""

    def __init__(self, n=8):
        from oracle import pyoracle as O
        self.c = c = raw_case("A")
        self.chan = [[CU.colour_channels(g, 71, i, eye) for eye, g in enumerate(c.raw[i])] for i in range(n)]
        self.gray = [tuple(np.ascontiguousarray(CU.gray_of_rgb(*ch[:3])) for ch in pair) for pair in self.chan]
        self.rect = [(O.remap_bilinear(a, *c.maps[0]), O.remap_bilinear(b, *c.maps[1])) for a, b in self.gray]

    def colour(self, i, fmt):
        return tuple(CU.pack(*ch, fmt) for ch in self.chan[i])


_RAWC = []


def raw_colour():
    if not _RAWC:
        _RAWC.append(RawColour())
    return _RAWC[0]


def test_colour_then_rectify(hip_lib, oracle_lib):
    """rectifiers attached to a BGR8 handle: plane(eye, 3) is the converted raw image, plane(eye, 2) the oracle's remap OF THAT, byte for byte; four frames
    against the oracle chain on those"""
    rc = raw_colour()
    c = rc.c
    hip = colour_system(hip_lib, c.prm, CU.BGR8)
    rl, rr = c.rectifiers(hip_lib)
    assert hip.set_rectifiers(rl, rr) == 0, hip.last_error()
    orc = c.oracle()
    for i in range(4):
        Ro, to = orc.track(*rc.rect[i])
        R, t = hip.track(*rc.colour(i, CU.BGR8))
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        if i == 0:
            for eye in (0, 1):
                assert_plane(hip.plane(eye, 3), rc.gray[0][eye], c.W, c.H, c.pitch, f"converted, eye {eye}")
                assert_plane(hip.plane(eye, 2), rc.rect[0][eye], c.W, c.H, c.pitch, f"rectified, eye {eye}")


# ---- 6. batches ----------------------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_of_colour_gray_raw_and_absent(hip_lib, oracle_lib):
    """four sequences of two image sizes in one chain, three steps in flight: 0 = RGB8; 1 = gray; 2 = BGRA8 with rectifiers; 3 = RGB8, sitting out steps 2
    and 5.  Each against its own oracle chain: state and pose of every step it has a frame in, all counters behind the last"""
    from oracle import pyoracle as O
    a, b, rc = stereo_seq(71, (621, 187)), stereo_seq(32, (613, 185)), raw_colour()
    prms = [a.prm, b.prm, rc.c.prm, b.prm]
    batch = hip_lib.LvtBatch(prms)
    assert batch.set_pixel_format(0, CU.RGB8) == 0 and batch.set_pixel_format(2, CU.BGRA8) == 0 and batch.set_pixel_format(3, CU.RGB8) == 0, batch.last_error()
    assert [batch.pixel_format(s) for s in range(4)] == [CU.RGB8, CU.GRAY8, CU.BGRA8, CU.RGB8]
    rl, rr = rc.c.rectifiers(hip_lib)
    assert batch.set_rectifiers(2, rl, rr) == 0, batch.last_error()
    nsteps = 8
    which = [[k, k, k, None] for k in range(nsteps)]
    f3 = 0
    for k in range(nsteps):
        if k not in (2, 5):
            which[k][3] = f3
            f3 += 1
    gray1 = [tuple(np.ascontiguousarray(g) for g in b.world.render_stereo(i)) for i in range(nsteps)]
    images = [a.gray, gray1, rc.rect, b.gray]               # what each sequence's oracle is given
    dev0 = [[device_colour(img, 1 + (i + e) % 3) for e, img in enumerate(a.colour(i, CU.RGB8))] for i in range(nsteps)]
    dev1 = [device_gray([gray1[i][e] for i in range(nsteps)], b.W, b.H, b.pitch) for e in (0, 1)]
    dev2 = [[device_colour(img, 2 + e) for e, img in enumerate(rc.colour(i, CU.BGRA8))] for i in range(nsteps)]
    dev3 = [[device_colour(img, 3 - e, extra=0) for e, img in enumerate(b.colour(i, CU.RGB8))] for i in range(f3)]   # (tightly packed rows)

    def ptrs(s, i):
        if s == 1:
            return dev1[0][i].data_ptr(), dev1[1][i].data_ptr(), b.pitch
        d = (dev0, None, dev2, dev3)[s][i]
        assert d[0][2] == d[1][2]
        return d[0][1], d[1][1], d[0][2]
    got, inflight = [], 0
    for k in range(nsteps):
        p = [None if which[k][s] is None else ptrs(s, which[k][s]) for s in range(4)]
        rc_ = batch.track_device_async_mixed([x and x[0] for x in p], [x and x[1] for x in p], [q.H for q in (a, b, a, b)], [q.W for q in (a, b, a, b)],
                                             [x[2] if x else 0 for x in p])
        assert rc_ == 0, batch.last_error()
        inflight += 1
        if inflight >= 3:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    assert batch.last_error() == "", batch.last_error()
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


def test_uniform_rgbd_batch_with_one_colour_sequence(hip_lib, oracle_lib):
    """a uniform RGB-D batch of two: sequence 0 BGRA8 at an odd address and pitch, sequence 1 gray (one frame ahead), 16-bit depth"""
    import torch
    q = rgbd_seq()
    n = 6
    batch = hip_lib.LvtBatch(q.prm, 2, sensor_type=2)
    assert batch.set_pixel_format(0, CU.BGRA8) == 0, batch.last_error()
    refs = [q.chain(range(n)), q.chain(range(1, n + 1), images=q.raw_gray)]
    d16 = torch.from_numpy(np.stack(q.u16).view(np.int16)).cuda()
    dgray = device_gray(q.raw_gray, q.W, q.H, q.pitch)
    for k in range(n):
        keep = device_colour(q.colour(k, CU.BGRA8), 1 + k % 3)
        rc_ = batch.track_rgbd_device_async([keep[1], dgray[k + 1].data_ptr()], [d16[k].data_ptr(), d16[k + 1].data_ptr()], q.H, q.W, [keep[2], q.pitch], 2 * q.W,
                                            hip_lib.DEPTH_U16, SCALE)
        assert rc_ == 0, batch.last_error()
        R, t, st = batch.wait()
        assert batch.last_error() == "", batch.last_error()
        for s in range(2):
            assert st[s] == refs[s][k][2], f"sequence {s} step {k}: state {st[s]}"
            close_to(R[s], t[s], refs[s][k], f"sequence {s} step {k}")
            counts_equal(batch.counts(s), refs[s][k][3], f"sequence {s} step {k}")


def test_a_batch_with_more_colour_images_than_one_table_holds(hip_lib, oracle_lib):
    """33 RGB8 stereo sequences = 66 colour images: the step takes a second k_gray_frames launch (sequence 32's two images).  Sequence s starts at frame
    s % 3 of the world; three steps; sequences 0, 1, 31 and 32 against their oracle chains (state, pose, all counters), every sequence TRACKING"""
    q = stereo_seq(71, (621, 187))
    B, steps = 33, 3
    batch = hip_lib.LvtBatch(q.prm, B)
    for s in range(B):
        assert batch.set_pixel_format(s, CU.RGB8) == 0, batch.last_error()
    dev = [[device_colour(img, 1 + (i + e) % 3) for e, img in enumerate(q.colour(i, CU.RGB8))] for i in range(steps + 2)]
    refs = [q.chain(range(o, o + steps)) for o in range(3)]
    batch.profile_enable(True)
    for k in range(steps):
        fr = [dev[k + s % 3] for s in range(B)]
        batch.track_device_async([f[0][1] for f in fr], [f[1][1] for f in fr], q.H, q.W, dev[0][0][2])
        R, t, st = batch.wait()
        assert batch.last_error() == "", batch.last_error()
        assert list(st) == [2] * B, (k, list(st))
        for s in (0, 1, 31, 32):
            ref = refs[s % 3][k]
            assert st[s] == ref[2]
            close_to(R[s], t[s], ref, f"sequence {s} step {k}")
            counts_equal(batch.counts(s), ref[3], f"sequence {s} step {k}")
    assert dict(_profile_of(batch))["k_gray_frames"] == steps   # (the slot times a step's first launch)


# ---- 7. refusals and switching -------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(hip_lib, oracle_lib, tmp_path):
    """every refusal returns -1 with a reason, and the handle tracks its next GRAY frame as the oracle does"""
    import torch
    q = stereo_seq(71, (621, 187))
    L = hip_lib.load_library()
    gray = q.gray   # (any gray frames: the oracle gets the same ones)

    said = []

    def refused(h, rc):
        assert rc == -1 and h.last_error() != "", (rc, h.last_error())
        said.append(h.last_error())

    hip, orc = hip_lib.LvtSystem.create(q.prm, 1), q.oracle()

    def diff():   # (a refusal's text stays in last_error until the next report: it is the one line of the diff that is expected)
        return [m for m in diff_frame(hip, orc) if not (said and m == "hip error: " + said[-1])]

    def next_gray(i):
        Ro, to = orc.track(*gray[i])
        R, t = hip.track(*gray[i])
        msgs = diff()
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"gray frame {i}")
        assert hip.pixel_format() == CU.GRAY8 and hip.plane(0, 3).size == 0

    for k, bad in enumerate((-1, 5, 99)):
        refused(hip, hip.set_pixel_format(bad))                            # an unknown format
        assert "unknown pixel format" in hip.last_error()
        next_gray(k)
    refused(hip, L.lvt_amd_batch_set_pixel_format(hip._h, 0, CU.RGB8))     # the batch call on a handle that is not a batch
    next_gray(3)
    dev = device_gray([gray[4][0], gray[4][1]], q.W, q.H, q.pitch)
    hip.track_device_async(dev[0].data_ptr(), dev[1].data_ptr(), q.H, q.W, q.pitch)
    refused(hip, hip.set_pixel_format(CU.RGB8))                            # a frame in flight
    assert "in flight" in hip.last_error()
    R, t, st = hip.wait_status()
    orc.track(*gray[4])
    assert st == orc.status == 2 and not diff()
    next_gray(5)
    assert hip.set_pixel_format(CU.RGB8) == 0, hip.last_error()              # everything collected: accepted
    before = hip.host_stats()["enqueued"]
    col = device_colour(q.colour(6, CU.RGB8)[0], 1, extra=0)
    hip.track_device_async(col[1], col[1], q.H, q.W, q.W * 3 - 1)           # a pitch that does not hold a row of colour pixels
    assert "pitch" in hip.last_error() and hip.host_stats()["enqueued"] == before
    said.append(hip.last_error())
    assert hip.set_pixel_format(CU.GRAY8) == 0
    next_gray(6)

    seat = hip_lib.LvtSystem.create(q.prm, 1, pooled=True)
    assert seat.ordering() == "pooled"
    refused(seat, seat.set_pixel_format(CU.RGB8))                          # a pooled seat
    q.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    autos = [hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1) for _ in range(2)]
    assert autos[0].ordering() == "pooled"
    refused(autos[0], autos[0].set_pixel_format(CU.RGB8))                  # an automatic seat
    ref = q.chain()
    for h in (seat, autos[0]):
        assert h.pixel_format() == CU.GRAY8
        for i in range(2):
            R, t = h.track(*gray[i])
            close_to(R, t, ref[i], f"a seat's gray frame {i}")
        assert h.get_state() == 2
    seat.close()
    for h in autos:
        h.close()

    batch = hip_lib.LvtBatch(q.prm, 2)
    for seq in (-1, 2):
        refused(batch, batch.set_pixel_format(seq, CU.RGB8))               # seq out of range
        assert batch.pixel_format(seq) == -1
    refused(batch, L.lvt_amd_set_pixel_format(batch._h, CU.RGB8))          # the solo call on a batch
    refused(batch, batch.set_pixel_format(1, 7))
    assert L.lvt_amd_get_pixel_format(None, 0) == -1
    dev = torch.stack([device_gray([gray[i][0], gray[i][1]], q.W, q.H, q.pitch) for i in range(2)])
    for i in range(2):
        batch.track_device_async([dev[i, 0].data_ptr()] * 2, [dev[i, 1].data_ptr()] * 2, q.H, q.W, q.pitch)
        R, t, st = batch.wait()
        for s in range(2):
            assert st[s] == 2
            close_to(R[s], t[s], ref[i], f"batch sequence {s} gray frame {i}")
            counts_equal(batch.counts(s), ref[i][3], f"batch sequence {s} gray frame {i}")
    assert batch.last_error() == said[-1], batch.last_error()   # (the last refusal's text stays; the frames added no report)


@pytest.mark.parametrize("route", ["lvt_track", "track_async"])
def test_switching_between_colour_and_gray(hip_lib, oracle_lib, route):
    """set_pixel_format(RGB8), three colour frames, collect; set_pixel_format(GRAY8), three gray frames: ONE oracle chain covers all six.  Through the
    asynchronous host route as well: its pinned staging is sized by the format"""
    q = stereo_seq(71, (621, 187))
    ref = q.chain()
    hip, orc = colour_system(hip_lib, q.prm, CU.RGB8), q.oracle()
    for i in range(6):
        if i == 3:
            assert hip.set_pixel_format(CU.GRAY8) == 0, hip.last_error()
            assert hip.pixel_format() == CU.GRAY8
        imgs = q.colour(i, CU.RGB8) if i < 3 else q.gray[i]
        orc.track(*q.gray[i])
        if route == "lvt_track":
            R, t = hip.track(*imgs)
        else:
            assert hip.track_async(*imgs) == 0, hip.last_error()
            R, t, st = hip.wait_status()
            assert st == 2
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, ref[i], f"frame {i}")
        assert (hip.plane(0, 3).size != 0) == (i < 3)
    with pytest.raises((ValueError, AssertionError)):
        hip.track(*q.colour(0, CU.RGB8))                                    # a colour image on a gray handle raises in the binding
    assert hip.set_pixel_format(CU.RGB8) == 0, hip.last_error()
    assert hip.plane(0, 3).size == 0                                        # a colour handle whose last frame was a gray one: nothing was converted


def test_a_set_is_a_use_of_an_lvt_create_handle(hip_lib, oracle_lib, tmp_path):
    """lvt_create, set_pixel_format, a second lvt_create with the same parameters: the first handle keeps its own chain, and converts"""
    q = stereo_seq(71, (621, 187))
    q.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    first = hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1)
    assert first.set_pixel_format(CU.RGBA8) == 0, first.last_error()
    second = hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1)
    assert first.ordering() != "pooled"
    first.track(*q.colour(0, CU.RGBA8))
    assert_plane(first.plane(0, 3), q.gray[0][0], q.W, q.H, q.pitch, "eye 0")
    second.close(); first.close()


# ---- 8. launches -----------------------------------------------------------------------------------------------------------------------------------
def _profile_of(h):
    return [(name, calls) for name, _ms, calls in h.profile_read()]


def test_launch_accounting(hip_lib, oracle_lib):
    """a gray handle has no k_gray_frames row (and no k_rectify_frames row: the rows of a plain handle); a colour handle reports exactly one k_gray_frames
    call per frame and nothing else changes; a batch with four colour sequences reports one call per step"""
    q = stereo_seq(71, (621, 187))
    plain = hip_lib.LvtSystem.create(q.prm, 1)
    plain.profile_enable(True)
    for i in range(4):
        plain.track(*q.gray[i])
    rows = _profile_of(plain)
    assert rows and not [n for n, _ in rows if "k_gray_frames" in n or "k_rectify_frames" in n], rows
    assert dict(rows)["k_score"] == 4
    plain.close()   # (a handle created beside a live one orders its streams with events: other rows)

    hip = colour_system(hip_lib, q.prm, CU.RGB8)
    hip.profile_enable(True)
    for i in range(4):
        hip.track(*q.colour(i, CU.RGB8))
    prof = _profile_of(hip)
    assert dict(prof)["k_gray_frames"] == 4, prof
    assert [(n, k) for n, k in prof if n != "k_gray_frames"] == rows, (prof, rows)
    hip.close()

    batch = hip_lib.LvtBatch(q.prm, 4)
    for s in range(4):
        assert batch.set_pixel_format(s, CU.RGB8) == 0, batch.last_error()
    batch.profile_enable(True)
    for i in range(2):
        dev = [device_colour(img, 1 + e) for e, img in enumerate(q.colour(i, CU.RGB8))]
        batch.track_device_async([dev[0][1]] * 4, [dev[1][1]] * 4, q.H, q.W, dev[0][2])
        batch.wait()
    prof = dict(_profile_of(batch))
    assert prof["k_gray_frames"] == 2 and prof["k_score"] == 2, prof
    assert batch.last_error() == "", batch.last_error()
