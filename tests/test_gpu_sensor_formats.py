"""SENSOR FORMATS on the GPU: the stage entry (lvt_amd_convert_sensor_device) against the numpy restatement byte for byte, and sequences of Bayer, YUV 4:2:2
and 16-bit planes against the UNCHANGED oracle, which is fed the numpy-converted frames (sensor_util).  No expected value comes from the library under test.
Frames in flight together are held to the oracle by state and pose, frame by frame, and by the complete parity_util.diff_frame behind the last one; the
synchronous routes run diff_frame behind every frame."""
import ctypes
import itertools

import numpy as np
import pytest

import colour_util as CU
import sensor_util as SU
from parity_util import diff_frame
from test_gpu_raw_frames import close_to, counts_equal, _run_async as run_async
from test_gpu_colour_frames import stereo_seq, rgbd_seq, device_colour, assert_plane, SCALE

pytestmark = pytest.mark.gpu

GUARD = 0xA5
WIDTHS = (2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127)
HEIGHTS = (2, 3, 5, 33)
OFFSETS = (0, 1, 3, 5, 7, 16)            # four odd; MONO16 (even addresses only) takes twice these
FORMAT_IDS = [SU.NAMES[f] for f in SU.FORMATS]


def record(hip_lib, rec):
    return hip_lib.SensorFormat(**rec.fields())


def raw_bytes(plane):
    """a sensor's plane as (H, row bytes) uint8"""
    a = np.ascontiguousarray(plane)
    return a.view(np.uint8).reshape(a.shape[0], -1)


def random_plane(rng, fmt, w, h):
    if fmt == SU.MONO16:
        return rng.integers(0, 65536, size=(h, w), dtype=np.uint16)
    return rng.integers(0, 256, size=(h, w * SU.BPP[fmt]), dtype=np.uint8)


# ---- the stage entry -----------------------------------------------------------------------------------------------------------------------------
def stage(hip_lib, plane, rec, offset=0, src_pitch=None, dst_extra=0, pad=255):
    """a sensor's plane through lvt_amd_convert_sensor_device.  The source lies `offset` bytes past a 256-byte boundary, rows src_pitch apart, every byte that
    is no sample holds `pad`; the destination has dst_pitch = the width rounded up to 4, + dst_extra, and GUARD bytes in front of and behind it.  Returns
    (the destination rows (h, dst_pitch), the window) after checking the guards and that the source is as it was."""
    import torch
    src = raw_bytes(plane)
    h, row = src.shape
    w = row // SU.BPP[rec.format]
    src_pitch = row if src_pitch is None else src_pitch
    dst_pitch = (w + 3) // 4 * 4 + dst_extra
    d0 = 256
    s0 = (d0 + h * dst_pitch + 256 + 255) // 256 * 256 + offset
    buf = np.full(s0 + h * src_pitch + 64, pad, np.uint8)
    buf[:s0 - offset] = GUARD
    np.lib.stride_tricks.as_strided(buf[s0:], shape=(h, row), strides=(src_pitch, 1))[:] = src
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 256 == 0
    rc, win = hip_lib.convert_sensor_device(record(hip_lib, rec), t.data_ptr() + s0, src_pitch, w, h, t.data_ptr() + d0, dst_pitch)
    assert rc == 0, hip_lib.last_call_error()
    out = t.cpu().numpy()
    assert (out[:d0] == GUARD).all() and (out[d0 + h * dst_pitch:s0 - offset] == GUARD).all(), "guard bytes around the destination were written"
    assert np.array_equal(out[s0 - offset:], buf[s0 - offset:]), "the source or the bytes around it were written"
    return out[d0:d0 + h * dst_pitch].reshape(h, dst_pitch), win


def check(hip_lib, plane, rec, what, **kw):
    got, win = stage(hip_lib, plane, rec, **kw)
    want, wwin = SU.convert(plane, rec)
    w = want.shape[1]
    assert win == wwin, f"{what}: window {win}, numpy {wwin}"
    bad = np.argwhere(got[:, :w] != want)
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at {tuple(bad[0])}: hip {got[tuple(bad[0])]} numpy {want[tuple(bad[0])]}"
    assert not got[:, w:].any(), f"{what}: the padding columns are not zero"


def placements(fmt, row):
    """(offset, pitch) of a source whose rows are `row` bytes: every offset with an odd pitch and with a multiple of 16 (MONO16: even offsets, a pitch that is
    2 mod 4 in place of the odd one) -- offsets 0 and 16 with the latter take the dword loads, everything else the single-sample loads"""
    m16 = fmt == SU.MONO16
    for off in OFFSETS:
        yield (2 * off if m16 else off), ((row + 2) | 2 if m16 else (row + 1) | 1)
        yield (2 * off if m16 else off), (row + 15) // 16 * 16 + 16


def record_for(fmt, n):
    if fmt != SU.MONO16:
        return SU.Record(fmt)
    if n % 2:
        return SU.Record(fmt, auto_window=1, lo_permille=n % 7 * 10, hi_permille=n % 5 * 10, min_span=1 + 37 * (n % 11))
    return SU.Record(fmt, lo=1000 * (n % 9), hi=20000 + 4000 * (n % 11))


@pytest.mark.parametrize("fmt", SU.FORMATS, ids=FORMAT_IDS)
def test_stage_sizes_and_placements(hip_lib, fmt):
    """every width and height of the lists with random samples; every byte between and around the rows holds 255 (a dark image for Bayer: a neighbour taken from
    beyond a row's end shows).  The twelve placements rotate through the sizes with a stride of 5, co-prime to the 4 heights and to 12: every width and every
    height meets odd and 16-byte pitches, aligned and unaligned offsets; MONO16 alternates fixed and auto windows"""
    rng = np.random.default_rng(300 + fmt)
    for n, (w, h) in enumerate(itertools.product(WIDTHS, HEIGHTS)):
        plane = random_plane(rng, fmt, w, h)
        if fmt in SU.BAYER:
            plane >>= 3
        pl = list(placements(fmt, w * SU.BPP[fmt]))
        off, pitch = pl[(n * 5) % len(pl)]
        check(hip_lib, plane, record_for(fmt, n), f"{SU.NAMES[fmt]} w {w} h {h} offset {off} pitch {pitch}", offset=off, src_pitch=pitch, dst_extra=4 * (n % 3))


@pytest.mark.parametrize("fmt", SU.FORMATS, ids=FORMAT_IDS)
def test_stage_every_placement_gives_the_same_bytes(hip_lib, fmt):
    """one random image, 65 x 33 and 127 x 5, at every offset and both kinds of pitch"""
    rng = np.random.default_rng(fmt)
    for w, h in ((65, 33), (127, 5), (8, 2)):
        plane = random_plane(rng, fmt, w, h)
        for off, pitch in placements(fmt, w * SU.BPP[fmt]):
            check(hip_lib, plane, record_for(fmt, 2), f"{SU.NAMES[fmt]} {w} x {h} offset {off} pitch {pitch}", offset=off, src_pitch=pitch)


@pytest.mark.parametrize("fmt", SU.BAYER, ids=[SU.NAMES[f] for f in SU.BAYER])
def test_stage_bayer_contents(hip_lib, fmt):
    """all 0, all 255 (the largest sum), a flat field of every level, and the mosaic of a constant colour, on the dword and on the byte path"""
    flat = np.repeat(np.arange(256, dtype=np.uint8), 6).reshape(256, 6)        # rows of one level each are NOT flat fields: planted per image below
    for off in (0, 1):
        for name, img in (("zeros", np.zeros((9, 13), np.uint8)), ("ones", np.full((9, 13), 255, np.uint8)), ("ramp", flat),
                          ("constant colour", SU.mosaic(np.full((6, 10), 200, np.uint8), np.full((6, 10), 17, np.uint8), np.full((6, 10), 99, np.uint8), fmt))):
            check(hip_lib, img, SU.Record(fmt), f"{name} offset {off}", offset=off, src_pitch=(img.shape[1] + 15) // 16 * 16)
    for v in (0, 1, 127, 128, 254, 255):
        got, _ = stage(hip_lib, np.full((4, 8), v, np.uint8), SU.Record(fmt))
        assert (got == v).all(), v
    got, _ = stage(hip_lib, SU.mosaic(np.full((6, 8), 255, np.uint8), np.zeros((6, 8), np.uint8), np.zeros((6, 8), np.uint8), fmt), SU.Record(fmt))
    assert (got == 76).all()                                                   # colour_util.KNOWN_ANSWERS: pure red


@pytest.mark.parametrize("lo,hi", SU.EVERY_VALUE_WINDOWS)
def test_stage_mono16_every_value(hip_lib, lo, hi):
    """the 256 x 256 image of every v in 0 ... 65 535: the proof of the division by hi - lo, on the dword path and on the 16-bit path"""
    img = SU.every_value_image()
    for off, pitch in ((0, 512), (2, 518)):
        check(hip_lib, img, SU.Record(SU.MONO16, lo=lo, hi=hi), f"window {lo} ... {hi} offset {off}", offset=off, src_pitch=pitch)


def test_stage_mono16_every_span_at_its_edges(hip_lib):
    """spans 1 ... 65535 sampled densely at both ends and sparsely between, each with the values around its own rounding steps: v = lo + k for k around the
    points where the quotient changes"""
    rng = np.random.default_rng(8)
    spans = sorted(set(list(range(1, 600)) + list(range(65000, 65536)) + [int(s) for s in rng.integers(600, 65000, 300)]))
    for d in spans[::7]:
        lo = int(rng.integers(0, 65536 - d))
        img = rng.integers(max(0, lo - 3), min(65535, lo + d + 3) + 1, size=(4, 64), dtype=np.uint16)
        check(hip_lib, img, SU.Record(SU.MONO16, lo=lo, hi=lo + d), f"span {d} lo {lo}")


PLANTED = SU.planted_histograms()


@pytest.mark.parametrize("name,img,cfg,want", PLANTED, ids=[p[0] for p in PLANTED])
def test_stage_auto_window_on_planted_histograms(hip_lib, name, img, cfg, want):
    rec = SU.Record(SU.MONO16, auto_window=1, lo_permille=cfg[0], hi_permille=cfg[1], min_span=cfg[2])
    for off, pitch in ((0, (2 * img.shape[1] + 15) // 16 * 16), (2, 2 * img.shape[1] + 2)):
        got, win = stage(hip_lib, img, rec, offset=off, src_pitch=pitch)
        assert win == want, (name, win, want)
        assert np.array_equal(got[:, :img.shape[1]], SU.map16(img, *want))


def test_stage_auto_window_over_several_workgroups(hip_lib):
    """640 x 480 and 641 x 479 (an odd width: every row ends in a single sample): 75 workgroups of the histogram kernel; twice in a row -- the second call finds
    no trace of the first"""
    rng = np.random.default_rng(12)
    for w, h in ((640, 480), (641, 479)):
        img = np.clip(rng.normal(21000, 400, size=(h, w)), 0, 65535).astype(np.uint16)
        img[rng.integers(0, h, 50), rng.integers(0, w, 50)] = 65535              # hot pixels: above the window
        rec = SU.Record(SU.MONO16, auto_window=1, lo_permille=10, hi_permille=10, min_span=64)
        for _ in range(2):
            check(hip_lib, img, rec, f"{w} x {h}", offset=2, src_pitch=2 * w + 6)
        check(hip_lib, img, rec, f"{w} x {h} aligned", src_pitch=(2 * w + 15) // 16 * 16)


def test_stage_refusals(hip_lib):
    import torch
    t = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    F = hip_lib.SensorFormat
    m16 = F(SU.MONO16, lo=0, hi=100)
    for args, word in (((F(SU.RGGB), 0, 16, 16, 16, p, 16), "NULL"), ((None, p, 16, 16, 16, p + 4096, 16), "NULL"),
                       ((F(SU.NONE), p, 16, 16, 16, p + 4096, 16), "LVT_AMD_SENSOR_NONE"), ((F(5), p, 16, 16, 16, p + 4096, 16), "unknown sensor format 5"),
                       ((F(SU.RGGB), p, 16, 0, 16, p + 4096, 16), "side"), ((F(SU.RGGB), p, 16, 16, 16385, p + 4096, 16), "side"),
                       ((F(SU.RGGB), p, 16, 1, 16, p + 4096, 16), "width = 1"), ((F(SU.GBRG), p, 16, 16, 1, p + 4096, 16), "height = 1"),
                       ((F(SU.MONO16, lo=5, hi=5), p, 32, 16, 16, p + 4096, 16), "hi = 5"), ((F(SU.MONO16, auto_window=1, lo_permille=500), p, 32, 16, 16, p + 4096, 16), "lo_permille = 500"),
                       ((F(SU.YUYV), p, 31, 16, 16, p + 4096, 16), "source pitch"), ((m16, p + 1, 32, 16, 16, p + 4096, 16), "even"), ((m16, p, 33, 16, 16, p + 4096, 16), "even"),
                       ((F(SU.UYVY), p, 32, 16, 16, p + 4096, 12), "destination"), ((F(SU.UYVY), p, 32, 16, 16, p + 4096, 18), "destination"),
                       ((F(SU.UYVY), p, 32, 16, 16, p + 4097, 16), "destination")):
        assert hip_lib.convert_sensor_device(*args) == (-1, None), args
        assert word in hip_lib.last_call_error() and hip_lib.last_call_error().endswith("(nothing was launched)"), hip_lib.last_call_error()
    assert not t.cpu().numpy().any()


# ---- sequences -------------------------------------------------------------------------------------------------------------------------------------
class SensorStereo:
    """world 71 at 621 x 187 (the colour tests'), as each sensor would deliver it: the planes, the numpy conversion of each and the windows"""

    def __init__(self, n=8):
        self.q = q = stereo_seq(71, (621, 187), n)
        self.prm, self.W, self.H, self.pitch, self.n = q.prm, q.W, q.H, q.pitch, n
        self.world_gray = [tuple(np.ascontiguousarray(g) for g in q.world.render_stereo(i)) for i in range(n)]
        self._made = {}

    def frames(self, rec_key):
        """(record, raw planes [i][eye], converted gray [i][eye], windows [i][eye])"""
        if rec_key not in self._made:
            q, n = self.q, self.n
            if rec_key in SU.BAYER:
                rec = SU.Record(rec_key)
                raw = [tuple(SU.mosaic(*c[:3], rec_key) for c in q.chan[i]) for i in range(n)]
            elif rec_key in (SU.YUYV, SU.UYVY):
                rec = SU.Record(rec_key)
                raw = [tuple(SU.yuv422_of_gray(g, rec_key, 10 * i + e) for e, g in enumerate(self.world_gray[i])) for i in range(n)]
            elif rec_key == "thermal":
                rec = SU.THERMAL
                raw = [tuple(SU.thermal(g, 2 * i + e) for e, g in enumerate(self.world_gray[i])) for i in range(n)]
            else:
                rec = SU.Record(SU.MONO16, lo=19990, hi=20790)
                raw = [tuple(SU.thermal(g, 2 * i + e) for e, g in enumerate(self.world_gray[i])) for i in range(n)]
            conv = [tuple(SU.convert(p, rec) for p in pair) for pair in raw]
            self._made[rec_key] = (rec, raw, [tuple(c[0] for c in pair) for pair in conv], [tuple(c[1] for c in pair) for pair in conv])
        return self._made[rec_key]

    def oracle(self):
        return self.q.oracle()

    def chain(self, rec_key, frames=None):
        return self.q.chain(frames, images=self.frames(rec_key)[2])


_SS = []


def sensor_stereo():
    if not _SS:
        _SS.append(SensorStereo())
    return _SS[0]


def sensor_system(hip_lib, prm, rec, sensor=1):
    hip = hip_lib.LvtSystem.create(prm, sensor)
    assert hip.set_sensor_format(record(hip_lib, rec)) == 0, hip.last_error()
    got = hip.sensor_format()
    assert got is not None and {k: int(getattr(got, k)) for k in rec.fields()} == rec.fields()
    return hip


def device_sensor(plane, rec, offset, extra=None):
    """a sensor's plane in HBM, `offset` bytes past an aligned address with rows `extra` bytes longer than a row (None: 4 or 5, whichever makes the pitch
    odd): (owner, address, pitch)"""
    b = raw_bytes(plane)
    bpp = SU.BPP[rec.format]
    extra = (5 if b.shape[1] % 2 == 0 else 4) if extra is None else extra
    return device_colour(b.reshape(b.shape[0], b.shape[1] // bpp, bpp), offset, extra)


def check_async(s, key, hip, got):
    ref = s.chain(key)
    for i, (R, t, st) in enumerate(got):
        assert st == ref[i][2], f"frame {i}: state {st} oracle {ref[i][2]}"
        close_to(R, t, ref[i], f"frame {i}")
    orc = s.oracle()
    for i in range(len(got)):
        orc.track(*s.frames(key)[2][i])
    msgs = diff_frame(hip, orc)
    assert not msgs, msgs[:6]
    counts_equal(hip.counts(), ref[len(got) - 1][3], "last frame")


@pytest.mark.parametrize("key", [SU.RGGB, SU.UYVY, "thermal"], ids=["RGGB8", "UYVY", "MONO16-auto"])
def test_lvt_track(hip_lib, oracle_lib, key):
    """eight frames through lvt_track: the complete frame diff is empty behind every frame, plane 3 is the numpy conversion, the window numpy's"""
    s = sensor_stereo()
    rec, raw, conv, wins = s.frames(key)
    hip, orc = sensor_system(hip_lib, s.prm, rec), s.oracle()
    for i in range(8):
        Ro, to = orc.track(*conv[i])
        R, t = hip.track(*raw[i])
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        for eye in (0, 1):
            assert_plane(hip.plane(eye, 3), conv[i][eye], s.W, s.H, s.pitch, f"frame {i} eye {eye}")
            assert hip.sensor_window(eye) == wins[i][eye], (i, eye, hip.sensor_window(eye), wins[i][eye])
        assert hip.plane(0, 2).size == 0


def test_track_async_three_in_flight(hip_lib, oracle_lib):
    """BGGR host frames through lvt_amd_track_async, three in flight: the staging and the fused pull carry the mosaic"""
    s = sensor_stereo()
    rec, raw, conv, _ = s.frames(SU.BGGR)
    hip = sensor_system(hip_lib, s.prm, rec)

    def submit(i):
        assert hip.track_async(*raw[i]) == 0, hip.last_error()
    got = run_async(hip, submit, 8, 3)
    check_async(s, SU.BGGR, hip, got)
    hs = hip.host_stats()
    assert hs["async_host_frames"] == 8 and hs["pulls_carried_by_the_previous_frame"] > 0, hs


@pytest.mark.parametrize("key", [SU.GRBG, SU.YUYV, "fixed"], ids=["GRBG8", "YUYV", "MONO16-fixed"])
def test_device_planes_at_an_odd_address_and_pitch(hip_lib, oracle_lib, key):
    """planes in HBM read in place, three in flight: 1 ... 3 bytes past an aligned address with an odd pitch (MONO16: 2 bytes past, a row + 6)"""
    s = sensor_stereo()
    rec, raw, conv, _ = s.frames(key)
    hip = sensor_system(hip_lib, s.prm, rec)
    m16 = rec.format == SU.MONO16
    dev = [[device_sensor(p, rec, 2 if m16 else 1 + (i + e) % 3, 6 if m16 else None) for e, p in enumerate(raw[i])] for i in range(8)]
    assert m16 or dev[0][0][2] % 2 == 1

    def submit(i):
        hip.track_device_async(dev[i][0][1], dev[i][1][1], s.H, s.W, dev[i][0][2])
    got = run_async(hip, submit, 8, 3)
    assert hip.last_error() == "", hip.last_error()
    check_async(s, key, hip, got)


def test_external_corners(hip_lib, oracle_lib):
    """GBRG frames through lvt_track_with_external_corners, the corners taken from the oracle's detector on the converted gray: coordinates do not move"""
    from oracle import pyoracle as O
    s = sensor_stereo()
    rec, raw, conv, _ = s.frames(SU.GBRG)
    hip, orc = sensor_system(hip_lib, s.prm, rec), s.oracle()
    for i in range(6):
        cl = O.compute_features(conv[i][0], s.prm)[0].astype(np.float64)
        cr = O.compute_features(conv[i][1], s.prm)[0].astype(np.float64)
        Ro, to = orc.track_with_external_corners(conv[i][0], conv[i][1], cl, cr)
        R, t = hip.track_with_external_corners(*raw[i], cl, cr)
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"


def test_rgbd_with_bayer(hip_lib, oracle_lib):
    """the tum world at 322 x 242 as an RGGB mosaic + 16-bit depth: host frames three in flight, then device planes at an odd address one by one"""
    import torch
    from oracle import pyoracle as O
    q = rgbd_seq()
    rec = SU.Record(SU.RGGB)
    raw = [SU.mosaic(*q.chan[i][:3], SU.RGGB) for i in range(8)]
    conv = [SU.bayer_to_gray(m, SU.RGGB) for m in raw]
    ref = q.chain(range(8), images=conv)
    hip = sensor_system(hip_lib, q.prm, rec, 2)

    def submit(i):
        assert hip.track_async(raw[i], q.u16[i], depth_scale=SCALE) == 0, hip.last_error()
    got = run_async(hip, submit, 8, 3)
    for i, (R, t, st) in enumerate(got):
        assert st == ref[i][2], f"frame {i}: state {st}"
        close_to(R, t, ref[i], f"frame {i}")
    orc = O.Oracle(q.prm, 2)
    for i in range(8):
        orc.track_rgbd(conv[i], q.f32[i])
    msgs = diff_frame(hip, orc)
    assert not msgs, msgs[:6]
    assert_plane(hip.plane(0, 3), conv[7], q.W, q.H, q.pitch, "last frame")
    hip.close()
    hip, orc = sensor_system(hip_lib, q.prm, rec, 2), O.Oracle(q.prm, 2)
    d16 = torch.from_numpy(np.stack(q.u16[:6]).view(np.int16)).cuda()
    for i in range(6):
        keep = device_sensor(raw[i], rec, 1 + i % 3)
        assert hip.track_rgbd_device_async(keep[1], d16[i].data_ptr(), q.H, q.W, keep[2], 2 * q.W, hip_lib.DEPTH_U16, SCALE) == 0, hip.last_error()
        R, t, st = hip.wait_status()
        Ro, to = orc.track_rgbd(conv[i], q.f32[i])
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        assert orc.status == 2 == st


def test_bayer_then_rectify(hip_lib, oracle_lib):
    """rectifiers on a GRBG handle: plane 3 is the converted raw image, plane 2 the oracle's remap OF THAT; six frames against the oracle on those"""
    from oracle import pyoracle as O
    from test_gpu_colour_frames import raw_colour
    rc = raw_colour()
    c = rc.c
    raw = [tuple(SU.mosaic(*ch[:3], SU.GRBG) for ch in rc.chan[i]) for i in range(6)]
    conv = [tuple(SU.bayer_to_gray(m, SU.GRBG) for m in pair) for pair in raw]
    rect = [(O.remap_bilinear(a, *c.maps[0]), O.remap_bilinear(b, *c.maps[1])) for a, b in conv]
    hip = sensor_system(hip_lib, c.prm, SU.Record(SU.GRBG))
    rl, rr = c.rectifiers(hip_lib)
    assert hip.set_rectifiers(rl, rr) == 0, hip.last_error()
    orc = c.oracle()
    for i in range(6):
        Ro, to = orc.track(*rect[i])
        R, t = hip.track(*raw[i])
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        if i == 0:
            for eye in (0, 1):
                assert_plane(hip.plane(eye, 3), conv[0][eye], c.W, c.H, c.pitch, f"converted, eye {eye}")
                assert_plane(hip.plane(eye, 2), rect[0][eye], c.W, c.H, c.pitch, f"rectified, eye {eye}")


def test_yuyv_then_reduce(hip_lib, oracle_lib):
    """kitti 620 x 188 from 1240 x 376 YUYV planes: convert, then reduce; the oracle gets reduce_util's reduction of the luma"""
    import reduce_util as RU
    q = RU.large_world("kitti", 3, (1240, 376), 2)
    hip = hip_lib.LvtSystem.create(q.prm, 1)
    assert hip.set_reduction(q.reduction()) == 0, hip.last_error()
    assert hip.set_sensor_format(hip_lib.SENSOR_YUYV) == 0, hip.last_error()
    orc = q.oracle()
    for i in range(6):
        raw = tuple(SU.yuv422_of_gray(g, SU.YUYV, 2 * i + e) for e, g in enumerate(q.large[i]))
        Ro, to = orc.track(*q.small[i])
        R, t = hip.track(*raw)
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
    assert np.array_equal(hip.plane(0, 3)[:, :q.fW], q.large[5][0]) and np.array_equal(hip.plane(1, 9)[:, :q.W], q.small[5][1])


def test_mono16_auto_then_equalise(hip_lib, oracle_lib):
    """the thermal world with the auto window and CLAHE behind it: the oracle gets clahe_util's equalisation of the numpy-mapped frames"""
    import clahe_util as CL
    s = sensor_stereo()
    rec, raw, conv, wins = s.frames("thermal")
    eq = [tuple(np.ascontiguousarray(CL.clahe(g, (8, 4), 3.0)) for g in pair) for pair in conv[:6]]
    hip, orc = sensor_system(hip_lib, s.prm, rec), s.oracle()
    assert hip.set_equalisation(tiles=(8, 4), clip_limit=3.0) == 0, hip.last_error()
    for i in range(6):
        Ro, to = orc.track(*eq[i])
        R, t = hip.track(*raw[i])
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        assert (hip.sensor_window(0), hip.sensor_window(1)) == wins[i]


def test_mixed_batch_of_bayer_mono16_auto_plain_and_absent(hip_lib, oracle_lib):
    """0 = RGGB; 1 = MONO16 with the auto window; 2 = plain gray planes; 3 = UYVY, sitting out steps 1 and 3; the MONO16 sequence sits out
    step 4.  Three steps in flight.  Each against its own oracle chain: state and pose of every step it has a frame in, all counters behind the last;
    sensor_window behind every collected step equals numpy's for the frame of that step, and is None behind the step the MONO16 sequence sat out of"""
    import torch
    from oracle import pyoracle as O
    s = sensor_stereo()
    B, nsteps = 4, 6
    batch = hip_lib.LvtBatch([s.prm] * B)
    keys = [SU.RGGB, "thermal", None, SU.UYVY]
    for k, key in enumerate(keys):
        if key is not None:
            assert batch.set_sensor_format(k, record(hip_lib, s.frames(key)[0])) == 0, batch.last_error()
    assert batch.sensor_format(2) is None and batch.sensor_format(1).auto_window == 1 and batch.sensor_format(3).format == SU.UYVY
    which = [[k, None, k, None] for k in range(nsteps)]
    f1 = f3 = 0
    for k in range(nsteps):
        if k != 4:
            which[k][1] = f1
            f1 += 1
        if k not in (1, 3):
            which[k][3] = f3
            f3 += 1
    images = [s.frames(SU.RGGB)[2], s.frames("thermal")[2], s.world_gray, s.frames(SU.UYVY)[2]]
    dev = {}
    for k, key in enumerate(keys):
        if key is not None:
            rec, raw = s.frames(key)[:2]
            m16 = rec.format == SU.MONO16
            dev[k] = [[device_sensor(p, rec, 2 if m16 else 1 + e, 6 if m16 else None) for e, p in enumerate(raw[i])] for i in range(nsteps)]
    plain = torch.zeros((nsteps, 2, s.H, s.pitch), dtype=torch.uint8, device="cuda")
    for i in range(nsteps):
        for e in (0, 1):
            plain[i, e, :, :s.W] = torch.from_numpy(s.world_gray[i][e]).cuda()

    def ptrs(k, i):
        if k == 2:
            return plain[i, 0].data_ptr(), plain[i, 1].data_ptr(), s.pitch
        d = dev[k][i]
        return d[0][1], d[1][1], d[0][2]
    got, inflight, windows = [], 0, []
    for k in range(nsteps):
        p = [None if which[k][q] is None else ptrs(q, which[k][q]) for q in range(B)]
        rc = batch.track_device_async_mixed([x and x[0] for x in p], [x and x[1] for x in p], [s.H] * B, [s.W] * B, [x[2] if x else 0 for x in p])
        assert rc == 0, batch.last_error()
        inflight += 1
        if inflight >= 3:
            got.append(batch.wait()); inflight -= 1
            windows.append([batch.sensor_window(1, e) for e in (0, 1)])
    while inflight:
        got.append(batch.wait()); inflight -= 1
        windows.append([batch.sensor_window(1, e) for e in (0, 1)])
    assert batch.last_error() == "", batch.last_error()
    want = [(None, None) if which[k][1] is None else s.frames("thermal")[3][which[k][1]] for k in range(nsteps)]
    assert want[4] == (None, None) and want[5] == s.frames("thermal")[3][4]
    assert [tuple(w) for w in windows] == want, (windows, want)
    assert batch.sensor_window(0) is None and batch.sensor_window(2) is None and batch.sensor_window(3) is None
    for q in range(B):
        orc = O.Oracle(s.prm, 1)
        for k in range(nsteps):
            if which[k][q] is None:
                continue
            Ro, to = orc.track(*images[q][which[k][q]])
            R, t, st = got[k]
            assert orc.status == 2, f"sequence {q} step {k}: the oracle is not TRACKING"
            assert st[q] == orc.status, f"sequence {q} step {k}: state {st[q]}"
            close_to(R[q], t[q], (np.array(Ro), np.array(to)), f"sequence {q} step {k}")
        counts_equal(batch.counts(q), orc.counts(), f"sequence {q} after the last step")


def test_uniform_batch_with_more_images_than_one_table_holds(hip_lib, oracle_lib):
    """25 MONO16-auto stereo sequences = 50 images: a step takes a second launch of each of the three kernels.  Sequence q starts at frame q % 6; two steps"""
    s = sensor_stereo()
    rec, raw, conv, wins = s.frames("thermal")
    B, steps = 25, 2
    batch = hip_lib.LvtBatch(s.prm, B)
    for q in range(B):
        assert batch.set_sensor_format(q, record(hip_lib, rec)) == 0, batch.last_error()
    dev = [[device_sensor(p, rec, 2, 6) for p in raw[i]] for i in range(8)]
    refs = [s.q.chain(range(q % 6, q % 6 + steps), images=conv) for q in range(B)]
    batch.profile_enable(True)
    for k in range(steps):
        fr = [dev[q % 6 + k] for q in range(B)]
        batch.track_device_async([f[0][1] for f in fr], [f[1][1] for f in fr], s.H, s.W, dev[0][0][2])
        R, t, st = batch.wait()
        assert batch.last_error() == "", batch.last_error()
        for q in range(B):
            ref = refs[q][k]
            assert st[q] == ref[2] == 2, (q, k, st[q])
            close_to(R[q], t[q], ref, f"sequence {q} step {k}")
            counts_equal(batch.counts(q), ref[3], f"sequence {q} step {k}")
            assert tuple(batch.sensor_window(q, e) for e in (0, 1)) == wins[q % 6 + k], (q, k)
    prof = dict(profile_of(batch))
    assert prof["k_sensor_frames"] == prof["k_sensor_hist"] == prof["k_sensor_levels"] == steps   # (a slot times a step's first launch)


# ---- launches, switching, state --------------------------------------------------------------------------------------------------------------------
def profile_of(h):
    return [(name, calls) for name, _ms, calls in h.profile_read()]


SENSOR_ROWS = ("k_sensor_frames", "k_sensor_hist", "k_sensor_levels")


def test_launch_counts(hip_lib, oracle_lib):
    """a plain handle has none of the three rows; a fixed-format handle reports exactly one k_sensor_frames call per frame and nothing else changes; the two
    auto launches appear only with auto_window; after SENSOR_NONE the handle tracks plain frames to the oracle's bits with the plain handle's launches"""
    s = sensor_stereo()
    plain = hip_lib.LvtSystem.create(s.prm, 1)
    plain.profile_enable(True)
    for i in range(4):
        plain.track(*s.world_gray[i])
    rows = profile_of(plain)
    assert rows and not [n for n, _ in rows if n in SENSOR_ROWS], rows
    assert dict(rows)["k_score"] == 4
    plain.close()   # (a handle created beside a live one orders its streams with events: other rows)

    for key, extra in ((SU.RGGB, {"k_sensor_frames": 4}), ("fixed", {"k_sensor_frames": 4}),
                       ("thermal", {"k_sensor_frames": 4, "k_sensor_hist": 4, "k_sensor_levels": 4})):
        rec, raw = s.frames(key)[:2]
        hip = sensor_system(hip_lib, s.prm, rec)
        hip.profile_enable(True)
        for i in range(4):
            hip.track(*raw[i])
        prof = profile_of(hip)
        assert {n: k for n, k in prof if n in SENSOR_ROWS} == extra, (key, prof)
        assert [(n, k) for n, k in prof if n not in SENSOR_ROWS] == rows, (prof, rows)
        hip.close()

    back = sensor_system(hip_lib, s.prm, s.frames("thermal")[0])
    back.track(*s.frames("thermal")[1][0])
    back.reset()
    assert back.set_sensor_format(None) == 0, back.last_error()
    assert back.sensor_format() is None and back.sensor_window(0) is None
    back.profile_enable(True)
    orc = s.oracle()
    for i in range(4):
        orc.track(*s.world_gray[i])
        back.track(*s.world_gray[i])
        msgs = diff_frame(back, orc)
        assert not msgs, (i, msgs[:6])
        assert back.plane(0, 3).size == 0
    assert profile_of(back) == rows, (profile_of(back), rows)


def test_snapshots_do_not_hold_the_property_and_reset_leaves_it(hip_lib, oracle_lib):
    s = sensor_stereo()
    rec, raw, conv, _ = s.frames(SU.RGGB)
    plain, hip = hip_lib.LvtSystem.create(s.prm, 1), sensor_system(hip_lib, s.prm, rec)
    for i in range(3):
        plain.track(*conv[i])
        hip.track(*raw[i])
    a, b = plain.snapshot(), hip.snapshot()
    assert a.to_bytes() == b.to_bytes()
    assert plain.restore(b) == 0, plain.last_error()
    assert plain.sensor_format() is None                              # (a snapshot taken from a Bayer handle brings no format)
    assert hip.restore(a) == 0 and hip.sensor_format().format == SU.RGGB  # (... and one from a plain handle takes none away)
    a.close(); b.close()
    hip.reset()
    assert hip.sensor_format().format == SU.RGGB
    orc = s.oracle()
    for i in range(3):
        Ro, to = orc.track(*conv[i])
        R, t = hip.track(*raw[i])
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_the_contracts_order(hip_lib, oracle_lib, tmp_path):
    import torch
    s = sensor_stereo()
    L = hip_lib.load_library()
    F = hip_lib.SensorFormat
    rec, raw, conv, _ = s.frames(SU.RGGB)
    said = []

    def refused(h, rc, *words):
        assert rc == -1 and h.last_error().endswith("(nothing was changed)"), (rc, h.last_error())
        for w in words:
            assert w in h.last_error(), (w, h.last_error())
        said.append(h.last_error())

    hip, orc = hip_lib.LvtSystem.create(s.prm, 1), s.oracle()
    nxt = [0]

    def next_frame(sensor=False):
        i = nxt[0]
        nxt[0] += 1
        Ro, to = orc.track(*conv[i])
        R, t = hip.track(*(raw[i] if sensor else conv[i]))
        msgs = [m for m in diff_frame(hip, orc) if not (said and m == "hip error: " + said[-1])]
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")

    # the handle's kind, ahead of the value
    seat = hip_lib.LvtSystem.create(s.prm, 1, pooled=True)
    refused(seat, seat.set_sensor_format(F(5)), "pooled")
    s.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    autos = [hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1) for _ in range(2)]
    assert autos[0].ordering() == "pooled"
    refused(autos[0], autos[0].set_sensor_format(F(SU.RGGB)), "pooled")
    assert seat.sensor_format() is None and seat.sensor_window(0) is None
    seat.close()
    for h in autos:
        h.close()
    # the spelling
    refused(hip, L.lvt_amd_batch_set_sensor_format(hip._h, 5, ctypes.byref(F(5))), "lvt_amd_batch_set_sensor_format on a handle that is not a batch")
    batch = hip_lib.LvtBatch(s.prm, 2)
    refused(batch, L.lvt_amd_set_sensor_format(batch._h, ctypes.byref(F(5))), "lvt_amd_batch_set_sensor_format")
    # seq
    for seq in (-1, 2):
        refused(batch, batch.set_sensor_format(seq, F(5)), f"no sequence {seq}")
        with pytest.raises(IndexError):
            batch.sensor_format(seq)
        with pytest.raises(IndexError):
            batch.sensor_window(seq)
    with pytest.raises(IndexError):
        batch.sensor_window(0, 2)
    # the record
    refused(hip, L.lvt_amd_set_sensor_format(hip._h, None), "NULL")
    for bad in (5, 7, 99, 1, 20, 33, -1):
        refused(hip, hip.set_sensor_format(F(bad)), f"unknown sensor format {bad}")
    refused(hip, hip.set_sensor_format(F(SU.MONO16, auto_window=2)), "auto_window = 2")
    refused(hip, hip.set_sensor_format(F(SU.MONO16, lo=-1, hi=10)), "lo = -1")
    refused(hip, hip.set_sensor_format(F(SU.MONO16, lo=10, hi=10)), "hi = 10")
    refused(hip, hip.set_sensor_format(F(SU.MONO16, lo=10, hi=65536)), "hi = 65536")
    refused(hip, hip.set_sensor_format(F(SU.MONO16, auto_window=1, lo_permille=500)), "lo_permille = 500")
    refused(hip, hip.set_sensor_format(F(SU.MONO16, auto_window=1, hi_permille=-1)), "hi_permille = -1")
    refused(hip, hip.set_sensor_format(F(SU.MONO16, auto_window=1, min_span=0)), "min_span = 0")
    refused(hip, hip.set_sensor_format(F(SU.MONO16, auto_window=1, min_span=65536)), "min_span = 65536")
    assert hip.sensor_format() is None
    next_frame()
    # the mutual exclusion with colour, both ways
    assert hip.set_pixel_format(CU.RGB8) == 0
    refused(hip, hip.set_sensor_format(F(SU.RGGB)), "colour pixel format")
    assert hip.set_sensor_format(None) == 0                               # (nothing to unset: accepted, as GRAY8 on a gray handle is)
    assert hip.set_pixel_format(CU.GRAY8) == 0
    assert hip.set_sensor_format(F(SU.RGGB)) == 0, hip.last_error()
    refused(hip, hip.set_pixel_format(CU.BGRA8), "sensor format")
    assert hip.set_pixel_format(CU.GRAY8) == 0 and hip.pixel_format() == CU.GRAY8
    assert hip.set_sensor_format(None) == 0 and hip.sensor_format() is None
    next_frame()
    # frames in flight, behind the record
    dev = torch.zeros((2, s.H, s.pitch), dtype=torch.uint8, device="cuda")
    for e in (0, 1):
        dev[e, :, :s.W] = torch.from_numpy(conv[nxt[0]][e]).cuda()
    hip.track_device_async(dev[0].data_ptr(), dev[1].data_ptr(), s.H, s.W, s.pitch)
    refused(hip, hip.set_sensor_format(F(7)), "unknown sensor format 7")
    refused(hip, hip.set_sensor_format(F(SU.RGGB)), "in flight")
    _, _, st = hip.wait_status()
    orc.track(*conv[nxt[0]])
    nxt[0] += 1
    assert st == orc.status == 2
    assert hip.set_sensor_format(F(SU.RGGB)) == 0, hip.last_error()
    next_frame(sensor=True)

    # per frame, on the Bayer handle and on a MONO16 one
    def frame_refused(h, call, *words):
        before = h.host_stats()["enqueued"]
        call()
        assert h.host_stats()["enqueued"] == before and h.last_error() != "", h.last_error()
        for w in words:
            assert w in h.last_error(), (w, h.last_error())
        said.append(h.last_error())
    i = nxt[0]
    frame_refused(hip, lambda: hip.track(raw[i][0][:-1], raw[i][1][:-1]), "size")
    big = device_sensor(raw[i][0], rec, 1)
    frame_refused(hip, lambda: hip.track_device_async(big[1], big[1], s.H, s.W, s.W - 1), "pitch")
    next_frame(sensor=True)
    m = sensor_system(hip_lib, s.prm, SU.Record(SU.MONO16, lo=0, hi=1000))
    t16 = device_sensor(s.frames("fixed")[1][0][0], SU.Record(SU.MONO16), 2, 6)
    frame_refused(m, lambda: m.track_device_async(t16[1], t16[1], s.H, s.W, 2 * s.W - 2), "pitch")     # does not hold a row
    frame_refused(m, lambda: m.track_device_async(t16[1], t16[1], s.H, s.W, 2 * s.W + 5), "pitch")     # odd
    frame_refused(m, lambda: m.track_device_async(t16[1] + 1, t16[1], s.H, s.W, 2 * s.W + 6), "pitch")  # an odd address
    mb = hip_lib.LvtBatch(s.prm, 2)
    assert mb.set_sensor_format(1, F(SU.MONO16, lo=0, hi=1000)) == 0
    assert mb.track_device_async_mixed([None, t16[1] + 1], [None, t16[1]], [s.H] * 2, [s.W] * 2, [0, t16[2]]) == -1 and "even" in mb.last_error(), mb.last_error()
    # a Bayer format on frames under 2 pixels: refused by the stage entry (test_stage_refusals); no tracker is that small
    q = rgbd_seq()
    rg = sensor_system(hip_lib, q.prm, SU.Record(SU.MONO16, lo=0, hi=255), 2)
    g16 = device_sensor(q.raw_gray[0].astype(np.uint16), SU.Record(SU.MONO16), 1, 6)
    d = torch.ones((q.H, q.W), dtype=torch.float32, device="cuda")
    assert rg.track_rgbd_device_async(g16[1], d.data_ptr(), q.H, q.W, g16[2], 4 * q.W) == -1 and "even" in rg.last_error(), rg.last_error()
    assert rg.track_rgbd_device_async(g16[1] + 1, d.data_ptr(), q.H, q.W, 2 * q.W - 2, 4 * q.W) == -1 and "hold a row" in rg.last_error(), rg.last_error()


def test_a_set_is_a_use_of_an_lvt_create_handle(hip_lib, oracle_lib, tmp_path):
    s = sensor_stereo()
    rec, raw = s.frames(SU.RGGB)[:2]
    s.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    first = hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1)
    assert first.set_sensor_format(record(hip_lib, rec)) == 0, first.last_error()
    second = hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1)
    assert first.ordering() != "pooled"
    first.track(*raw[0])
    assert first.last_error() == "", first.last_error()
    second.close(); first.close()
