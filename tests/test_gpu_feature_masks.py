"""FEATURE MASKS on the GPU: lvt_amd_set_mask / lvt_amd_batch_set_mask and their _device forms, the launch k_mask_features between the gather step and BRIEF,
lvt_amd_get_mask_stats, plane 7 and the stage entry lvt_amd_mask_features.  No expected value comes from this library: the rule is restated in numpy
(mask_util.keep_rule, held to hand-written cases by test_feature_masks.py) and the tracker is held to the UNCHANGED oracle through two equivalences --
  stereo: a masked frame equals Oracle.track_with_external_corners(L, R, cl, cr) with cl, cr the oracle detector's corners of each eye filtered by the rule
          (everything parity_util.diff_frame compares except the features' responses, which the oracle's external corners do not have: those are held to
          the detector's responses of the kept corners);
  RGB-D:  detected corners are integers, so a masked frame equals Oracle.track_rgbd(gray, where(mask != 0, depth, 0)), the complete diff_frame.
Every oracle chain is asserted TRACKING before anything is compared, every masked comparison asserts that its mask drops at least one feature in every frame
and eye (the bonnet and the checkerboard at least 10 %).  Frames in flight together are held by state and pose, frame by frame, and by the complete diff behind
the last one.  The worlds: kitti 71 at 621 x 187 and tum 0 at 322 x 242, 8 frames; oracle chains are computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import mask_util as MU
from parity_util import make_case, diff_frame, sparse_pair
from test_gpu_raw_frames import close_to, counts_equal, _run_async as run_async
from test_gpu_colour_frames import device_colour, device_gray, assert_plane

pytestmark = pytest.mark.gpu

N = 8


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
class Stereo:
    def __init__(self):
        self.world, self.prm, _ = make_case("kitti", 71, size=(621, 187))
        self.W, self.H = self.world.W, self.world.H
        self.pitch = (self.W + 63) // 64 * 64
        self.frames = [tuple(np.ascontiguousarray(a) for a in self.world.render_stereo(i)) for i in range(N)]
        self.masks = {k: f(self.W, self.H) for k, f in MU.MASKS.items()}
        self._chains = {}

    def oracle(self):
        from oracle import pyoracle as O
        return O.Oracle(self.prm, 1)

    def chain(self, left, right, n=N):
        """the oracle over the first n frames under the named masks (None: no mask for that eye): ([(R, t, state, counts)], the oracle behind the last frame,
        the last frame's responses); asserted TRACKING throughout"""
        key = (left, right, n)
        if key not in self._chains:
            orc, out, resp = self.oracle(), [], None
            share = max(MU.MIN_SHARE.get(left, 0.0), MU.MIN_SHARE.get(right, 0.0)) if left == right else 0.0
            for i in range(n):
                R, t, resp = MU.oracle_track_masked(orc, self.prm, *self.frames[i], self.masks.get(left), self.masks.get(right), f"frame {i}", share)
                out.append((np.array(R), np.array(t), orc.status, orc.counts()))
            assert [r[2] for r in out] == [2] * n, "the oracle is not TRACKING on every frame: an early LOST would hide a difference"
            print("oracle matches:", [r[3]["n_matches"] for r in out])
            self._chains[key] = (out, orc, resp)
        return self._chains[key]


class Rgbd:
    def __init__(self, overrides=None):
        self.world, self.prm, sensor = make_case("tum", 0, 1.0, overrides, (322, 242))
        assert sensor == 2
        self.W, self.H = self.world.W, self.world.H
        self.pitch = (self.W + 63) // 64 * 64
        self.frames = [tuple(np.ascontiguousarray(a) for a in self.world.render_rgbd(i)) for i in range(N)]
        self.masks = {k: f(self.W, self.H) for k, f in MU.MASKS.items()}

    def oracle(self):
        from oracle import pyoracle as O
        return O.Oracle(self.prm, 2)

    def track_oracle(self, orc, i, name):
        from oracle import pyoracle as O
        g, d = self.frames[i]
        m = self.masks[name]
        MU.dropped_share(O.detect_grid(g, self.prm)[0], m, f"frame {i}", MU.MIN_SHARE[name])
        return orc.track_rgbd(g, MU.masked_depth(d, m))


_ONCE = {}


def stereo():
    if "s" not in _ONCE:
        _ONCE["s"] = Stereo()
    return _ONCE["s"]


def rgbd(barrel=False):
    key = "barrel" if barrel else "r"
    if key not in _ONCE:
        _ONCE[key] = Rgbd({"k1": -0.25} if barrel else None)
    return _ONCE[key]


def masked_system(hip_lib, q, left, right, sensor=1):
    hip = hip_lib.LvtSystem.create(q.prm, sensor)
    assert hip.set_mask(q.masks.get(left), q.masks.get(right)) == 0, hip.last_error()
    return hip


class Follow:
    """an oracle that is fed frame by frame beside a handle (the synchronous routes): one oracle call per frame instead of a chain per comparison"""

    def __init__(self, q):
        self.q, self.orc, self.resp = q, q.oracle(), None

    def frame(self, i, left, right, share=0.0, images=None):
        L, R = images or self.q.frames[i]
        Ro, to, self.resp = MU.oracle_track_masked(self.orc, self.q.prm, L, R, self.q.masks.get(left) if isinstance(left, (str, type(None))) else left,
                                                   self.q.masks.get(right) if isinstance(right, (str, type(None))) else right, f"frame {i}", share)
        return np.array(Ro), np.array(to)

    def hold(self, hip, i, R, t, Ro, to, tracking=True, drop=()):
        if tracking:
            assert self.orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = [m for m in MU.diff_frame_but_resp(hip, self.orc, self.resp) if not any(d in m for d in drop)]
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (Ro, to), f"frame {i}")


# ---- 1. the stage entry against numpy, bit for bit --------------------------------------------------------------------------------------------
PATTERNS = ["keep all", "drop all", "alternate", "only the first", "only the last", "drop the first 1024", "random half"]
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 4096]


def wanted(pattern, n, rng):
    k = np.zeros(n, bool)
    if pattern == "keep all":
        k[:] = True
    elif pattern == "alternate":
        k[::2] = True
    elif pattern == "only the first":
        k[:1] = True
    elif pattern == "only the last":
        k[n - 1:] = True
    elif pattern == "drop the first 1024":
        k[1024:] = True
    elif pattern == "random half":
        k = rng.random(n) < 0.5
    return k


def stage_case(pattern, n, pitch, seed):
    """n features in a 64 x 48 image whose keep flags under a random mask ARE the pattern: a kept feature lies on a kept pixel, a dropped one on a masked pixel
    or -- one in four -- outside the image; one in three sits at a .5 fraction (k - 0.5 belongs to pixel k), others a quarter pixel off.  Every other array
    is random bits.  The mask is a view into rows of `pitch` bytes whose padding holds 255: a wrong pitch would keep what must go"""
    W, H = 64, 48
    rng = np.random.default_rng(seed)
    store = np.full((H, pitch), 255, np.uint8)
    mask = store[:, :W]
    mask[:] = np.where(rng.random((H, W)) < 0.5, rng.integers(1, 256, (H, W)), 0)
    on, off = np.argwhere(mask != 0), np.argwhere(mask == 0)
    want = wanted(pattern, n, rng)
    pix = np.where(want[:, None], on[rng.integers(0, len(on), n)], off[rng.integers(0, len(off), n)]) if n else np.zeros((0, 2), np.int64)
    frac = rng.choice(np.array([0.0, -0.5, 0.25, -0.25], np.float32), size=(n, 2), p=[0.35, 0.33, 0.16, 0.16])
    bx, by = pix[:, 1].astype(np.float32) + frac[:, 0], pix[:, 0].astype(np.float32) + frac[:, 1]
    outside = ~want & (rng.random(n) < 0.25)
    bx[outside] = rng.choice(np.array([-1.5, -7.0, W - 0.5, W, W + 9.25], np.float32), size=int(outside.sum()))
    far = outside & (rng.random(n) < 0.5)
    by[far] = rng.choice(np.array([-1.5, H - 0.5, H + 3.0], np.float32), size=int(far.sum()))
    assert np.array_equal(MU.keep_rule(bx, by, mask), want), "the inputs do not realise the pattern"
    f32 = [rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32) for _ in range(4)]   # x, y, resp, depth: any bits, NaNs included
    i16 = [rng.integers(-32768, 32768, n).astype(np.int16) for _ in range(2)]
    return mask, want, [f32[0], f32[1], f32[2], bx, by, f32[3], i16[0], i16[1]]


@pytest.mark.parametrize("pitch", [64, 67])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_stage_entry_equals_numpy_bit_for_bit(hip_lib, pattern, pitch):
    for n in SIZES:
        mask, want, arrays = stage_case(pattern, n, pitch, 1000 * pitch + n)
        assert mask.strides[0] == pitch
        got = hip_lib.mask_features(*arrays, mask)
        assert got[0] == int(want.sum()), (pattern, n, got[0], int(want.sum()))
        for name, a, g in zip(("x", "y", "resp", "bx", "by", "depth", "hcx", "hcy"), arrays, got[1:]):
            bits = np.uint32 if a.dtype == np.float32 else np.int16
            assert np.array_equal(g[:got[0]].view(bits), a[want].view(bits)), (pattern, n, name)
            assert np.array_equal(g[got[0]:].view(bits), a[got[0]:].view(bits)), (pattern, n, name, "the tail was touched: the compaction is in place")


def test_stage_entry_refusals(hip_lib):
    mask, _, arrays = stage_case("alternate", 10, 64, 1)
    L = hip_lib.load_library()
    p = [a.ctypes.data_as(C.c_void_p) for a in arrays]
    m = np.ascontiguousarray(mask).ctypes.data_as(C.c_void_p)
    for args in ((4097, *p, m, 64, 48, 64), (-1, *p, m, 64, 48, 64), (10, *p, m, 64, 48, 63), (10, *p, None, 64, 48, 64), (10, *p, m, 0, 48, 64),
                 (10, *p[:4], None, *p[5:], m, 64, 48, 64)):
        assert L.lvt_amd_mask_features(*args) == -1
        err = L.lvt_amd_last_error(None).decode()
        assert err.startswith("lvt_amd_mask_features: ") and err.endswith("(nothing was changed)"), err


# ---- 2. one frame: a masked handle against an unmasked handle on the same images ---------------------------------------------------------------
@pytest.mark.parametrize("left,right", [("bonnet", "checkerboard"), ("ellipse", None)], ids=["two masks", "right eye NULL"])
def test_one_frame_equals_the_unmasked_handles_features_filtered(hip_lib, oracle_lib, left, right):
    q = stereo()
    plain = hip_lib.LvtSystem.create(q.prm, 1)
    plain.track(*q.frames[0])
    ref = [plain.features(eye) for eye in (0, 1)]
    assert plain.mask_stats() is None and plain.plane(0, 7).size == 0
    plain.close()
    hip = masked_system(hip_lib, q, left, right)
    assert hip.mask_stats() is None, "stats before the first frame under the mask"
    hip.track(*q.frames[0])
    assert hip.last_error() == "", hip.last_error()
    st = hip.mask_stats()
    for eye, name in enumerate((left, right)):
        xy, resp, desc = ref[eye]
        keep = MU.keep_rule(xy[:, 0], xy[:, 1], q.masks[name]) if name else np.ones(len(xy), bool)
        if name:
            assert 0 < keep.sum() < len(keep), "the mask drops nothing of this frame"
        xh, rh, dh = hip.features(eye)
        assert np.array_equal(xh, xy[keep]) and np.array_equal(rh, resp[keep]) and np.array_equal(dh, desc[keep]), f"eye {eye}"
        assert (st["kept"][eye], st["dropped"][eye]) == ((int(keep.sum()), int((~keep).sum())) if name else (0, 0)), (eye, st)
        if name:
            assert_plane(hip.plane(eye, 7), q.masks[name], q.W, q.H, q.pitch, f"mask of eye {eye}")
        else:
            assert hip.plane(eye, 7).size == 0
    c = hip.counts()
    assert (c["n_left"], c["n_right"]) == tuple(len(hip.features(e)[0]) for e in (0, 1))


# ---- 3. stereo sequences through lvt_track ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MU.MASKS))
def test_stereo_sequence_through_lvt_track(hip_lib, oracle_lib, name):
    q = stereo()
    hip, f = masked_system(hip_lib, q, name, name), Follow(q)
    for i in range(N):
        Ro, to = f.frame(i, name, name, MU.MIN_SHARE[name])
        R, t = hip.track(*q.frames[i])
        f.hold(hip, i, R, t, Ro, to)
        st = hip.mask_stats()
        assert st["kept"] == (hip.counts()["n_left"], hip.counts()["n_right"]) and min(st["dropped"]) > 0, st


# ---- 4. the routes ---------------------------------------------------------------------------------------------------------------------------
def check_async(q, hip, got, left, right):
    ref, orc, resp = q.chain(left, right, len(got))
    for i, (R, t, st) in enumerate(got):
        assert st == ref[i][2], f"frame {i}: state {st} oracle {ref[i][2]}"
        close_to(R, t, ref[i], f"frame {i}")
    msgs = MU.diff_frame_but_resp(hip, orc, resp)
    assert not msgs, msgs[:6]
    counts_equal(hip.counts(), ref[len(got) - 1][3], "last frame")


def test_masked_frames_through_track_async(hip_lib, oracle_lib):
    """lvt_amd_track_async on host frames, three in flight, the bonnet on both eyes"""
    q = stereo()
    hip = masked_system(hip_lib, q, "bonnet", "bonnet")

    def submit(i):
        assert hip.track_async(*q.frames[i]) == 0, hip.last_error()
    got = run_async(hip, submit, N, 3)
    check_async(q, hip, got, "bonnet", "bonnet")
    assert hip.host_stats()["async_host_frames"] == N


def test_device_planes_and_a_device_mask_at_an_odd_address(hip_lib, oracle_lib):
    """frames in HBM through lvt_amd_track_device_async, three in flight; the masks come through lvt_amd_set_mask_device from planes 1 and 3 bytes past an
    aligned address with a pitch of W + 67 and, in every byte that is no mask pixel, the OPPOSITE of the mask's majority: a copy that used one would show in
    plane 7 and in the features"""
    q = stereo()
    hip = hip_lib.LvtSystem.create(q.prm, 1)
    keep = [device_colour(q.masks[n][:, :, None], off, extra=67, guard=g) for n, off, g in (("checkerboard", 1, 255), ("ellipse", 3, 0))]
    assert keep[0][2] == q.W + 67 and keep[0][1] % 2 == 1 and keep[1][1] % 2 == 1
    assert hip.set_mask_device(keep[0][1], keep[0][2], keep[1][1], keep[1][2]) == 0, hip.last_error()
    for eye, n in enumerate(("checkerboard", "ellipse")):
        assert_plane(hip.plane(eye, 7), q.masks[n], q.W, q.H, q.pitch, f"mask of eye {eye}")
    dev = [device_gray([f[e] for f in q.frames], q.W, q.H, q.pitch) for e in (0, 1)]

    def submit(i):
        hip.track_device_async(dev[0][i].data_ptr(), dev[1][i].data_ptr(), q.H, q.W, q.pitch)
    got = run_async(hip, submit, N, 3)
    assert hip.last_error() == "", hip.last_error()
    check_async(q, hip, got, "checkerboard", "ellipse")


def planted(q, i, eye, mask):
    """the oracle detector's corners of a frame plus fractional corners planted on the checkerboard's vertical and horizontal edges, as fp32 values: at
    32 k - 0.5 (pixel 32 k) and at the float below it (pixel 32 k - 1), in x at rows well inside the image and in y likewise"""
    from oracle import pyoracle as O
    xyr = O.detect_grid(q.frames[i][eye], q.prm)[0]
    extra = []
    for k in range(2, 17):
        at = np.float32(32 * k) - np.float32(0.5)
        for y in (40.0, 70.25, 100.5, 140.0):
            extra += [(at, y), (np.nextafter(at, np.float32(0)), y)]
    for k in (2, 3, 4):
        at = np.float32(32 * k) - np.float32(0.5)
        for x in (50.0, 211.5, 400.25, 570.0):
            extra += [(x, at), (x, np.nextafter(at, np.float32(0)))]
    c = np.concatenate([xyr[:, :2], np.array(extra, np.float32)]).astype(np.float32)
    k = MU.keep_rule(c[:, 0], c[:, 1], mask)
    kp = k[len(xyr):]
    assert 0.3 < kp.mean() < 0.7 and np.all(kp[0::2] != kp[1::2]), "each planted pair straddles an edge"
    return c.astype(np.float64), c[k].astype(np.float64)


def test_external_corners_with_fractional_corners_on_mask_edges(hip_lib, oracle_lib):
    """lvt_track_with_external_corners on a masked handle: the corners are filtered by the same rule in the same coordinates, and the oracle is given the
    numpy-filtered lists.  The complete diff_frame (external corners have no response on either side)"""
    q = stereo()
    m = q.masks["checkerboard"]
    hip, orc = masked_system(hip_lib, q, "checkerboard", "checkerboard"), q.oracle()
    for i in range(N):
        (cl, kl), (cr, kr) = planted(q, i, 0, m), planted(q, i, 1, m)
        Ro, to = orc.track_with_external_corners(*q.frames[i], kl, kr)
        R, t = hip.track_with_external_corners(*q.frames[i], cl, cr)
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        xy = hip.features(0)[0]
        assert np.any(xy[:, 0] != np.rint(xy[:, 0])), "no planted corner among the features"


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("name", ["bonnet", "checkerboard"])
def test_rgbd_frames(hip_lib, oracle_lib, name, route):
    """gray + fp32 depth through lvt_amd_track_rgbd (host) and lvt_amd_track_rgbd_device_async (planes in HBM, collected one by one)"""
    import torch
    q = rgbd()
    hip, orc = masked_system(hip_lib, q, name, None, 2), q.oracle()
    if route == "device":
        g = device_gray([f[0] for f in q.frames], q.W, q.H, q.pitch)
        d = torch.from_numpy(np.stack([f[1] for f in q.frames])).cuda()
    for i in range(N):
        Ro, to = q.track_oracle(orc, i, name)
        if route == "host":
            R, t = hip.track(*q.frames[i])
        else:
            assert hip.track_rgbd_device_async(g[i].data_ptr(), d[i].data_ptr(), q.H, q.W, q.pitch, 4 * q.W) == 0, hip.last_error()
            R, t, _ = hip.wait_status()
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        st = hip.mask_stats()
        assert st["kept"] == (hip.counts()["n_left"], 0) and st["dropped"][0] > 0 and st["dropped"][1] == 0, st


def test_rgbd_with_a_barrel_lens(hip_lib, oracle_lib):
    """k1 < 0: the features are reported at undistorted coordinates, the mask is read at the raw pixel BRIEF samples at.  On every frame some kept feature's
    reported pixel is masked and its raw pixel is not: a filter on (x, y) would have dropped it"""
    q = rgbd(barrel=True)
    name = "checkerboard"
    assert q.prm.k1 < 0
    hip, orc = masked_system(hip_lib, q, name, None, 2), q.oracle()
    for i in range(N):
        Ro, to = q.track_oracle(orc, i, name)
        R, t = hip.track(*q.frames[i])
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        xy = hip.features(0)[0]
        assert np.any(xy != np.rint(xy)) and (~MU.keep_rule(xy[:, 0], xy[:, 1], q.masks[name])).sum() > 0, f"frame {i}: x, y and the raw pixel agree everywhere"


# ---- 5. together with the other properties -----------------------------------------------------------------------------------------------------
def test_colour_rectifiers_equalisation_and_a_mask(hip_lib, oracle_lib):
    """one handle takes BGR8 frames, rectifiers, an equalisation and masks: convert, remap, equalise, detect, gather, THEN the mask -- on the rectified grid.
    The oracle is fed the numpy-processed planes and the corners of ITS detector on them, filtered by the rule"""
    import clahe_util as CL
    import colour_util as CU
    from test_gpu_colour_frames import raw_colour
    rc = raw_colour()
    c = rc.c
    q = stereo()
    assert (c.W, c.H) == (q.W, q.H)
    eq = [tuple(CL.clahe(g, (4, 2), 4.0) for g in pair) for pair in rc.rect[:4]]
    hip = hip_lib.LvtSystem.create(c.prm, 1)
    assert hip.set_equalisation(hip_lib.Equalisation((4, 2), 4.0)) == 0 and hip.set_pixel_format(CU.BGR8) == 0, hip.last_error()
    rl, rr = c.rectifiers(hip_lib)
    assert hip.set_rectifiers(rl, rr) == 0, hip.last_error()
    assert hip.set_mask(q.masks["bonnet"], q.masks["checkerboard"]) == 0, hip.last_error()
    f = Follow(q)
    f.orc = c.oracle()
    for i in range(4):
        Ro, to = f.frame(i, "bonnet", "checkerboard", 0.10, images=eq[i])
        R, t = hip.track(*rc.colour(i, CU.BGR8))
        f.hold(hip, i, R, t, Ro, to)
    for eye in (0, 1):
        assert_plane(hip.plane(eye, 5), eq[3][eye], c.W, c.H, c.pitch, f"equalised, eye {eye}")


# ---- 6. batches ------------------------------------------------------------------------------------------------------------------------------
def solo_records(hip_lib, q, left, right, dev, frames):
    """[(R, t, state, counts)] of a solo handle with the masks over `frames` of the device planes"""
    hip = masked_system(hip_lib, q, left, right) if (left or right) else hip_lib.LvtSystem.create(q.prm, 1)
    out = []
    for i in frames:
        hip.track_device_async(dev[0][i].data_ptr(), dev[1][i].data_ptr(), q.H, q.W, q.pitch)
        R, t, st = hip.wait_status()
        out.append((R.copy(), t.copy(), st, hip.counts(), hip.mask_stats()))
    hip.close()
    return out


def test_mixed_batch_of_masked_plain_and_absent(hip_lib, oracle_lib):
    """three sequences in one chain, three steps in flight: 0 = 621 x 187 under the bonnet (left) and the checkerboard (right); 1 = 613 x 185, no mask; 2 =
    621 x 187 under the ellipse (left eye only), sitting out steps 2 and 4.  The masked sequences against the oracle chains, state and pose of every step and
    the counters behind the last; every sequence's poses, states and counters are those of a solo handle with the same masks, bit for bit.  Then a seventh
    step that sequences 1 and 2 sit out: the absent masked sequence reports no statistics (the step's launch did not run for it: its FeatCtl holds an older
    frame's counts), the present one the solo handle's"""
    q = stereo()
    bw, bprm, _ = make_case("kitti", 32, size=(613, 185))
    bframes = [tuple(np.ascontiguousarray(a) for a in bw.render_stereo(i)) for i in range(6)]
    bpitch = 640
    batch = hip_lib.LvtBatch([q.prm, bprm, q.prm])
    assert batch.set_mask(0, q.masks["bonnet"], q.masks["checkerboard"]) == 0 and batch.set_mask(2, q.masks["ellipse"], None) == 0, batch.last_error()
    assert batch.mask_stats(1) is None
    nsteps, which, f2, after = 6, [], 0, {}
    for k in range(6):
        which.append([k, k, None if k in (2, 4) else f2])
        f2 += 0 if k in (2, 4) else 1
    dev = [device_gray([f[e] for f in q.frames], q.W, q.H, q.pitch) for e in (0, 1)]
    devb = [device_gray([f[e] for f in bframes], 613, 185, bpitch) for e in (0, 1)]

    def ptr(s, i, e):
        return None if i is None else (devb if s == 1 else dev)[e][i].data_ptr()
    got, inflight = [], 0
    for k in range(nsteps):
        rc = batch.track_device_async_mixed([ptr(s, which[k][s], 0) for s in range(3)], [ptr(s, which[k][s], 1) for s in range(3)], [q.H, 185, q.H],
                                            [q.W, 613, q.W], [q.pitch, bpitch, q.pitch])
        assert rc == 0, batch.last_error()
        inflight += 1
        if inflight >= 3:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    assert batch.last_error() == "", batch.last_error()
    for s, (left, right) in ((0, ("bonnet", "checkerboard")), (2, ("ellipse", None))):
        steps = [k for k in range(nsteps) if which[k][s] is not None]
        ref, _, _ = q.chain(left, right, len(steps))
        solo = solo_records(hip_lib, q, left, right, dev, range(len(steps) + 1))   # (one frame more: the seventh step)
        solo, after[s] = solo[:-1], solo[-1]
        for j, k in enumerate(steps):
            R, t, st = got[k]
            assert st[s] == ref[j][2] == 2, f"sequence {s} step {k}: state {st[s]}"
            close_to(R[s], t[s], ref[j], f"sequence {s} step {k}")
            assert np.array_equal(R[s], solo[j][0]) and np.array_equal(t[s], solo[j][1]) and st[s] == solo[j][2], f"sequence {s} step {k}: not the solo handle's record"
        counts_equal(batch.counts(s), ref[-1][3], f"sequence {s} after the last step")
        assert {k: v for k, v in batch.counts(s).items() if k != "row_fallback"} == {k: v for k, v in solo[-1][3].items() if k != "row_fallback"}
        assert batch.mask_stats(s) == solo[-1][4] and sum(batch.mask_stats(s)["dropped"]) > 0
    from oracle import pyoracle as O
    orc = O.Oracle(bprm, 1)
    for k in range(nsteps):
        Ro, to = orc.track(*bframes[k])
        assert orc.status == 2 == got[k][2][1]
        close_to(got[k][0][1], got[k][1][1], (np.array(Ro), np.array(to)), f"sequence 1 step {k}")
    counts_equal(batch.counts(1), orc.counts(), "sequence 1 after the last step")
    assert batch.track_device_async_mixed([ptr(0, 6, 0), None, None], [ptr(0, 6, 1), None, None], [q.H, 185, q.H], [q.W, 613, q.W], [q.pitch, bpitch, q.pitch]) == 0, batch.last_error()
    batch.wait()
    assert batch.mask_stats(2) is None, ("a masked sequence that sat the last collected step out reports an older frame's counts", batch.mask_stats(2))
    assert batch.mask_stats(0) == after[0][4] and sum(batch.mask_stats(0)["dropped"]) > 0, (batch.mask_stats(0), after[0][4])


def test_uniform_batch_with_more_masked_sequences_than_one_table_holds(hip_lib, oracle_lib):
    """34 sequences, one table holds 32: sequence s runs under masks[s % 4] (bonnet both eyes / none / checkerboard left only / ellipse both), so both launches
    carry masked and unmasked slots and the second one starts at a sequence that is not its slot number.  Three steps, all in flight; every sequence's
    poses, states, counters and mask statistics are those of a solo handle with the same masks, bit for bit, and the first four follow the oracle"""
    q = stereo()
    B, kinds = 34, [("bonnet", "bonnet"), (None, None), ("checkerboard", None), ("ellipse", "ellipse")]
    batch = hip_lib.LvtBatch(q.prm, B)
    for s in range(B):
        left, right = kinds[s % 4]
        if left or right:
            assert batch.set_mask(s, q.masks.get(left), q.masks.get(right)) == 0, batch.last_error()
    dev = [device_gray([f[e] for f in q.frames[:3]], q.W, q.H, q.pitch) for e in (0, 1)]
    for i in range(3):
        batch.track_device_async([dev[0][i].data_ptr()] * B, [dev[1][i].data_ptr()] * B, q.H, q.W, q.pitch)
    got = [batch.wait() for _ in range(3)]
    assert batch.last_error() == "", batch.last_error()
    solo = [solo_records(hip_lib, q, left, right, dev, range(3)) for left, right in kinds]
    for s in range(B):
        rec = solo[s % 4]
        for i in range(3):
            R, t, st = got[i]
            assert np.array_equal(R[s], rec[i][0]) and np.array_equal(t[s], rec[i][1]) and st[s] == rec[i][2] == 2, f"sequence {s} step {i}"
        assert {k: v for k, v in batch.counts(s).items() if k != "row_fallback"} == {k: v for k, v in rec[2][3].items() if k != "row_fallback"}, f"sequence {s}"
        assert batch.mask_stats(s) == rec[2][4], f"sequence {s}"
    for s, (left, right) in enumerate(kinds):
        ref, _, _ = q.chain(left, right, 3)
        counts_equal(batch.counts(s), ref[2][3], f"sequence {s}")
        close_to(got[2][0][s], got[2][1][s], ref[2], f"sequence {s}")


# ---- 7. edges of behaviour -------------------------------------------------------------------------------------------------------------------
def test_an_all_255_mask_changes_no_bit(hip_lib, oracle_lib):
    q = stereo()
    full = np.full((q.H, q.W), 255, np.uint8)
    hip, plain = hip_lib.LvtSystem.create(q.prm, 1), hip_lib.LvtSystem.create(q.prm, 1)
    assert hip.set_mask(full, full) == 0, hip.last_error()
    for i in range(4):
        Ra, ta = hip.track(*q.frames[i])
        Rb, tb = plain.track(*q.frames[i])
        assert np.array_equal(Ra, Rb) and np.array_equal(ta, tb), f"frame {i}"
        for eye in (0, 1):
            for a, b in zip(hip.features(eye), plain.features(eye)):
                assert np.array_equal(a, b), f"frame {i} eye {eye}"
        assert hip.mask_stats()["dropped"] == (0, 0)
    assert hip.get_state() == plain.get_state() == 2
    assert hip.snapshot().to_bytes() == plain.snapshot().to_bytes(), "the snapshot of a masked handle knows its mask"


def test_an_all_zero_mask_loses_the_handle_for_good(hip_lib, oracle_lib):
    """two plain frames, an all-zero mask before the third: no features, LOST like the oracle on a frame without corners, and LOST after the unset"""
    q = stereo()
    hip, f = hip_lib.LvtSystem.create(q.prm, 1), Follow(q)
    zero, none = np.zeros((q.H, q.W), np.uint8), np.zeros((0, 2))
    for i in range(5):
        if i == 2:
            assert hip.set_mask(zero, zero) == 0, hip.last_error()
        if i == 3:
            assert hip.set_mask(None, None) == 0 and hip.mask_stats() is None
        if i == 2:
            Ro, to = f.orc.track_with_external_corners(*q.frames[i], none, none)
            f.resp = (np.zeros(0, np.float32),) * 2
        else:
            Ro, to = f.frame(i, None, None)
        R, t = hip.track(*q.frames[i])
        if i < 3:
            f.hold(hip, i, R, t, np.array(Ro), np.array(to), tracking=i < 2)
        assert hip.get_state() == f.orc.status == (2 if i < 2 else 3), (i, hip.get_state(), f.orc.status)
        counts_equal(hip.counts(), f.orc.counts(), f"frame {i}")
        if i == 2:
            st = hip.mask_stats()
            assert st["kept"] == (0, 0) and min(st["dropped"]) > 200, st


def test_the_retry_pass_under_a_mask(hip_lib, oracle_lib):
    """the nearly empty frame of parity_util.sparse_pair behind two tracked frames: fewer than 200 corners, so the detector runs again with the lowered
    threshold -- decided on the UNMASKED count -- and the bonnet then filters what the retry found; too few matches remain, and the handle is LOST where
    the oracle is.  (The oracle's external-corner route does not count retries: the two retry counters are held to its detector's own flag instead.)"""
    from oracle import pyoracle as O
    q = stereo()
    sp = tuple(np.ascontiguousarray(a) for a in sparse_pair(q.world, seed=3))
    flags = [O.detect_grid(a, q.prm)[1] for a in sp]
    assert flags == [1, 1], "the sparse pair does not take the retry"
    hip, f = masked_system(hip_lib, q, "bonnet", "bonnet"), Follow(q)
    for i, images in ((0, None), (1, None), (2, sp)):
        Ro, to = f.frame(i, "bonnet", "bonnet", 0.10, images=images)
        R, t = hip.track(*(images or q.frames[i]))
        f.hold(hip, i, R, t, Ro, to, tracking=images is None, drop=("count retry_",))
        c = hip.counts()
        assert (c["retry_left"], c["retry_right"]) == ((1, 1) if images else (0, 0)), c
        assert hip.get_state() == f.orc.status == (3 if images else 2)
    assert c["second_pass"] == 1 and hip.mask_stats()["dropped"][0] > 10


def test_set_unset_and_set_again_between_frames(hip_lib, oracle_lib):
    """frames 0 - 1 under the bonnet, 2 - 3 without a mask, 4 - 5 under the checkerboard (left) alone, 6 - 7 after lvt_amd_reset -- which keeps the mask --:
    ONE oracle chain covers the first six, a fresh one the last two"""
    q = stereo()
    hip, f = masked_system(hip_lib, q, "bonnet", "bonnet"), Follow(q)
    plan = [("bonnet", "bonnet")] * 2 + [(None, None)] * 2 + [("checkerboard", None)] * 4
    for i in range(N):
        if i in (2, 4):
            assert hip.set_mask(q.masks.get(plan[i][0]), q.masks.get(plan[i][1])) == 0, hip.last_error()
            assert hip.mask_stats() is None and (hip.plane(0, 7).size != 0) == (plan[i][0] is not None)
        if i == 6:
            hip.reset()
            f = Follow(q)
            assert_plane(hip.plane(0, 7), q.masks["checkerboard"], q.W, q.H, q.pitch, "the mask behind a reset")
        Ro, to = f.frame(i, *plan[i])
        R, t = hip.track(*q.frames[i])
        f.hold(hip, i, R, t, Ro, to)
        assert (hip.mask_stats() is None) == (plan[i] == (None, None))


def test_a_masked_handles_snapshot_continues_without_a_mask(hip_lib, oracle_lib):
    """four frames under the bonnet, a snapshot, applied to a plain handle: frames 4 - 7 there continue as the oracle does when its corners are no longer
    filtered; the masked handle goes on under its mask"""
    q = stereo()
    hip, plain = masked_system(hip_lib, q, "bonnet", "bonnet"), hip_lib.LvtSystem.create(q.prm, 1)
    f = Follow(q)
    for i in range(4):
        f.frame(i, "bonnet", "bonnet")
        hip.track(*q.frames[i])
    snap = hip.snapshot()
    assert plain.restore(snap) == 0, plain.last_error()
    assert plain.plane(0, 7).size == 0 and plain.mask_stats() is None
    for i in range(4, N):
        Ro, to = f.frame(i, None, None)
        R, t = plain.track(*q.frames[i])
        f.hold(plain, i, R, t, Ro, to)
    R, t = hip.track(*q.frames[4])
    close_to(R, t, q.chain("bonnet", "bonnet")[0][4], "the masked handle, frame 4")


# ---- 8. every refusal, in the contract's order ---------------------------------------------------------------------------------------------------
U = " (nothing was changed)"
RIDES = "a pooled handle (its frames ride a chain shared with other handles)" + U
HOST, DEV = "lvt_amd_set_mask: ", "lvt_amd_set_mask_device: "
TEXT = {
    "pooled": HOST + RIDES,
    "pooled device": DEV + RIDES,
    "solo call on a batch": HOST + "a batch handle takes its masks per sequence through lvt_amd_batch_set_mask" + U,
    "solo device call on a batch": DEV + "a batch handle takes its masks per sequence through lvt_amd_batch_set_mask_device" + U,
    "batch call on a solo": HOST + "lvt_amd_batch_set_mask on a handle that is not a batch (use lvt_amd_set_mask)" + U,
    "batch device call on a solo": DEV + "lvt_amd_batch_set_mask_device on a handle that is not a batch (use lvt_amd_set_mask_device)" + U,
    "seq 2": HOST + "no sequence 2 in this handle" + U,
    "seq -1": HOST + "no sequence -1 in this handle" + U,
    "pitch": DEV + "a mask pitch of 620 bytes on a sequence 621 pixels wide (pitch >= img_width)" + U,
    "right eye on RGB-D": HOST + "a right-eye mask on an RGB-D handle (it has one image: pass NULL for the right eye)" + U,
    "in flight": HOST + "frames in flight: set the mask before the first frame or after every frame has been collected" + U,
    "in flight device": DEV + "frames in flight: set the mask before the first frame or after every frame has been collected" + U,
}


def test_every_refusal_says_its_sentence_and_changes_nothing(hip_lib, oracle_lib, tmp_path):
    """each refusal returns -1 and leaves its complete sentence; where two objections apply the earlier one of the contract's order is named -- the handle's
    kind, the spelling, the sequence, the pitch, the right eye of an RGB-D handle, frames in flight --; and the masked handle goes on tracking, every frame
    against the oracle chain under the masks it had, bit for bit"""
    q, r = stereo(), rgbd()
    L, vp = hip_lib.load_library(), C.c_void_p
    m, other = q.masks["bonnet"], q.masks["checkerboard"]
    dm = device_colour(other[:, :, None], 0, extra=3)
    mp = np.ascontiguousarray(other).ctypes.data_as(vp)
    seen = []

    def refused(h, rc, key):
        assert rc == -1 and h.last_error() == TEXT[key], (key, rc, h.last_error())
        seen.append(key)

    assert L.lvt_amd_set_mask(None, mp, mp) == -1 and L.lvt_amd_set_mask_device(None, vp(dm[1]), dm[2], None, 0) == -1     # a bad handle: no report
    assert L.lvt_amd_get_mask_stats(None, 0, None) == -1
    hip, f, i = masked_system(hip_lib, q, "bonnet", "bonnet"), Follow(q), 0

    def next_frame():
        nonlocal i
        Ro, to = f.frame(i, "bonnet", "bonnet")
        R, t = hip.track(*q.frames[i])
        said = hip.last_error()
        msgs = [x for x in MU.diff_frame_but_resp(hip, f.orc, f.resp) if x != "hip error: " + said]
        assert not msgs and f.orc.status == 2, (i, msgs[:6])
        close_to(R, t, (Ro, to), f"frame {i}")
        assert_plane(hip.plane(1, 7), m, q.W, q.H, q.pitch, "the mask behind a refusal")
        i += 1

    next_frame()
    refused(hip, L.lvt_amd_batch_set_mask(hip._h, 0, mp, mp), "batch call on a solo")
    next_frame()
    refused(hip, L.lvt_amd_batch_set_mask(hip._h, 5, mp, mp), "batch call on a solo")                                       # the spelling before the sequence
    refused(hip, L.lvt_amd_batch_set_mask_device(hip._h, 0, vp(dm[1]), 620, None, 0), "batch device call on a solo")         # ... and before the pitch
    next_frame()
    refused(hip, hip.set_mask_device(dm[1], 620, dm[1], dm[2]), "pitch")
    refused(hip, hip.set_mask_device(dm[1], dm[2], dm[1], 620), "pitch")
    for call, key in ((lambda: hip.set_mask(other, other), "in flight"), (lambda: hip.set_mask(None, None), "in flight"),
                      (lambda: hip.set_mask_device(dm[1], dm[2], 0, 0), "in flight device"), (lambda: hip.set_mask_device(dm[1], 620, 0, 0), "pitch")):   # the pitch before the frames in flight
        dev = device_gray(list(q.frames[i]), q.W, q.H, q.pitch)
        hip.track_device_async(dev[0].data_ptr(), dev[1].data_ptr(), q.H, q.W, q.pitch)
        refused(hip, call(), key)
        Ro, to = f.frame(i, "bonnet", "bonnet")
        R, t, st = hip.wait_status()
        assert st == f.orc.status == 2
        close_to(R, t, (Ro, to), f"frame {i}")
        i += 1
    next_frame()
    hip.close()

    rg = masked_system(hip_lib, r, "bonnet", None, 2)
    orc = r.oracle()
    r.track_oracle(orc, 0, "bonnet"); rg.track(*r.frames[0])
    refused(rg, rg.set_mask(r.masks["bonnet"], r.masks["bonnet"]), "right eye on RGB-D")
    refused(rg, rg.set_mask(None, r.masks["bonnet"]), "right eye on RGB-D")
    r.track_oracle(orc, 1, "bonnet"); rg.track(*r.frames[1])
    msgs = [x for x in diff_frame(rg, orc) if not x.startswith("hip error: ")]
    assert not msgs and orc.status == 2, msgs[:6]
    rg.close()

    batch = hip_lib.LvtBatch(q.prm, 2)
    refused(batch, L.lvt_amd_set_mask(batch._h, mp, mp), "solo call on a batch")
    refused(batch, L.lvt_amd_set_mask_device(batch._h, vp(dm[1]), 620, None, 0), "solo device call on a batch")            # the spelling before the pitch
    refused(batch, batch.set_mask(2, other, other), "seq 2")
    refused(batch, batch.set_mask(-1, other, other), "seq -1")
    assert batch.set_mask_device(2, dm[1], 620) == -1 and batch.last_error() == TEXT["seq 2"].replace(HOST, DEV)             # the sequence before the pitch
    with pytest.raises(IndexError):
        batch.mask_stats(2)
    assert batch.set_mask(1, other, None) == 0 and batch.mask_stats(0) is None
    batch.close()

    seat = hip_lib.LvtSystem.create(q.prm, 1, pooled=True)
    q.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    autos = [hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1) for _ in range(2)]
    assert seat.ordering() == "pooled" and autos[0].ordering() == "pooled"
    for h in (seat, autos[0]):
        refused(h, h.set_mask(other, other), "pooled")
        refused(h, L.lvt_amd_batch_set_mask(h._h, 7, mp, mp), "pooled")                                                    # the kind before everything
        refused(h, h.set_mask_device(dm[1], 620), "pooled device")
        assert h.mask_stats() is None
        h.track(*q.frames[0])
        assert h.get_state() == 2
    for h in [seat] + autos:
        h.close()
    assert set(seen) == set(TEXT), set(TEXT) - set(seen)


def test_a_set_is_a_use_of_an_lvt_create_handle(hip_lib, oracle_lib, tmp_path):
    """lvt_create, set_mask, a second lvt_create with the same parameters: the first handle keeps its own chain, and its mask"""
    q = stereo()
    q.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    first = hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1)
    assert first.set_mask(q.masks["bonnet"], None) == 0, first.last_error()
    second = hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1)
    assert first.ordering() != "pooled"
    first.track(*q.frames[0])
    assert first.mask_stats()["dropped"][0] > 0
    assert_plane(first.plane(0, 7), q.masks["bonnet"], q.W, q.H, q.pitch, "eye 0")
    second.close(); first.close()


# ---- 9. launch accounting ------------------------------------------------------------------------------------------------------------------------
def _profile_of(h):
    return [(name, calls) for name, _ms, calls in h.profile_read()]


def test_launch_accounting(hip_lib, oracle_lib):
    """a handle that never set a mask has no k_mask_features row; a masked handle reports exactly one call per frame and every other row as the plain one"""
    q = stereo()
    plain = hip_lib.LvtSystem.create(q.prm, 1)
    plain.profile_enable(True)
    for i in range(4):
        plain.track(*q.frames[i])
    rows = _profile_of(plain)
    assert rows and not [n for n, _ in rows if "mask" in n], rows
    assert dict(rows)["k_score"] == 4
    plain.close()   # (a handle created beside a live one orders its streams with events: other rows)
    hip = masked_system(hip_lib, q, "bonnet", None)
    hip.profile_enable(True)
    for i in range(4):
        hip.track(*q.frames[i])
    prof = _profile_of(hip)
    assert dict(prof)["k_mask_features"] == 4, prof
    assert [(n, k) for n, k in prof if n != "k_mask_features"] == rows, (prof, rows)
    assert hip.set_mask(None, None) == 0
    hip.track(*q.frames[4])
    assert dict(_profile_of(hip))["k_mask_features"] == 4, "an unset mask still launches"
