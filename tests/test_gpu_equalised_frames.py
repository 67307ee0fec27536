"""DIM frames: an equalisation record per handle / per sequence of a batch (lvt_amd_set_equalisation / lvt_amd_batch_set_equalisation), CLAHE as two launches
at the head of the feature stage (k_clahe_lut, k_clahe_apply).  No expected value comes from this library: the stage is compared byte for byte with the numpy
restatement of the definition (clahe_util, held to hand-checked answers by tests/test_clahe.py), and the sequences are held to the ORACLE fed the
numpy-equalised frames -- parity_util.diff_frame behind every frame of the synchronous routes; state and pose frame by frame and a final diff_frame where
frames stay in flight.  Every oracle chain is asserted to be TRACKING on every frame before anything is compared, except where LOST is the point."""
import numpy as np
import pytest

import clahe_util as CL
import colour_util as CU
from parity_util import make_case, diff_frame
from test_clahe import SIZES, CLIPS, GAIN, OFFSET, TILES, CLIP
from test_gpu_raw_frames import close_to, counts_equal, _run_async as run_async
from test_gpu_colour_frames import SCALE, device_colour, device_gray, assert_plane, rgbd_seq, raw_colour, stereo_seq

pytestmark = pytest.mark.gpu

CONTENTS = ["random", "constant", "two_valued", "ramp", "all_255"]


# ---- 1. the stage alone ----------------------------------------------------------------------------------------------------------------------
def content(kind, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    if kind == "random":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "constant":
        return np.full((H, W), 77, np.uint8)
    if kind == "two_valued":
        return np.where(rng.random((H, W)) < 0.3, 40, 41).astype(np.uint8)
    if kind == "ramp":
        return ((np.arange(W)[None, :] + 3 * np.arange(H)[:, None]) % 256).astype(np.uint8)
    return np.full((H, W), 255, np.uint8)


_STAGE = {}


def stage_reference(W, H, tiles, kind, clip):
    """(image, tables, equalised image, [(excess, residual) per tile]) by numpy, computed once"""
    key = (W, H, tiles, kind, clip)
    if key not in _STAGE:
        img, stats = content(kind, W, H), []
        L = CL.luts(img, tiles, clip, stats)
        _STAGE[key] = (img, L, CL.apply(img, L, tiles, clip), stats)
    return _STAGE[key]


@pytest.mark.parametrize("size,tiles", SIZES, ids=[f"{w}x{h}-{a}x{b}" for (w, h), (a, b) in SIZES])
def test_the_stage_alone_equals_numpy(hip_lib, size, tiles):
    """lvt_amd_equalise_device on every content and clip limit: the source 0 ... 3 bytes past an aligned address with a pitch of W + 5 and 255 in every byte
    that is no pixel; the destination at a pitch beyond W inside a buffer of 0xAB: its W columns are numpy's bytes, its padding columns zero, every byte
    outside the plane untouched"""
    import torch
    W, H = size
    dpitch = (W + 3) // 4 * 4 + 8
    k = 0
    for kind in CONTENTS:
        for clip in CLIPS:
            img, _, want, _ = stage_reference(W, H, tiles, kind, clip)
            keep, src, spitch = device_colour(img[:, :, None], k % 4)
            assert spitch == W + 5 and src % 4 == k % 4
            dst = torch.full((256 + H * dpitch + 256,), 0xAB, dtype=torch.uint8, device="cuda")
            assert dst.data_ptr() % 4 == 0
            rc = hip_lib.equalise_device(hip_lib.Equalisation(tiles, clip), src, spitch, W, H, dst.data_ptr() + 256, dpitch)
            assert rc == 0, (kind, clip)
            got = dst.cpu().numpy()
            assert (got[:256] == 0xAB).all() and (got[256 + H * dpitch:] == 0xAB).all(), f"{kind} clip {clip}: bytes outside the plane were written"
            assert_plane(got[256:256 + H * dpitch].reshape(H, dpitch), want, W, H, dpitch, f"{kind} clip {clip} offset {k % 4}")
            k += 1


def test_the_stage_cases_cover_the_redistribution_rules():
    """over the cases above: a clip level at its floor of 1, a residual >= 129 (step == 1), a residual with step > 1 and a residual of 0"""
    seen = set()
    for (W, H), tiles in SIZES:
        for kind in CONTENTS:
            for clip in CLIPS:
                p = CL.plan(W, H, tiles, clip)
                if p["clip"] == 1:
                    seen.add("floor")
                for excess, residual in stage_reference(W, H, tiles, kind, clip)[3]:
                    if residual >= 129:
                        seen.add("step == 1")
                    elif residual > 0:
                        seen.add("step > 1" if 256 // residual > 1 else "step == 1")
                    else:
                        seen.add("residual == 0")
    assert {"floor", "step == 1", "step > 1", "residual == 0"} <= seen, seen


def test_the_stage_refuses_bad_arguments(hip_lib):
    import torch
    E = hip_lib.Equalisation
    a = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    b = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    ok = lambda cfg, sp=64, w=64, h=64, dp=64, off=0: hip_lib.equalise_device(cfg, a.data_ptr(), sp, w, h, b.data_ptr() + off, dp)   # noqa: E731
    assert ok(E((8, 8), 3.0)) == 0
    assert ok(E((17, 8), 3.0)) == -1 and ok(E((8, 8), 0.0)) == -1 and ok(E((8, 8), float("nan"))) == -1
    assert ok(E((8, 8), 3.0), sp=63) == -1 and ok(E((8, 8), 3.0), dp=62) == -1 and ok(E((8, 8), 3.0), w=60, dp=62) == -1
    assert ok(E((8, 8), 3.0), w=60, h=60, off=2) == -1 and ok(E((8, 8), 3.0), w=0) == -1


# ---- inputs of the sequence tests ------------------------------------------------------------------------------------------------------------
class DimWorld:
    """the world of tests/test_clahe.py: kitti seed 0 at 610 x 185, every frame dimmed to clip(rint(0.12 g + 10)); the numpy equalisation of the dimmed
    frames; the oracle's chains"""

    def __init__(self, n=6):
        self.world, self.prm, _ = make_case("kitti", 0, size=(610, 185))
        self.W, self.H, self.n = self.world.W, self.world.H, n
        self.pitch = (self.W + 63) // 64 * 64
        self.dim = [tuple(CL.dim(np.ascontiguousarray(g), GAIN, OFFSET) for g in self.world.render_stereo(i)) for i in range(n)]
        self.eq = [tuple(CL.clahe(g, TILES, CLIP) for g in pair) for pair in self.dim]
        self._chains = {}

    def oracle(self):
        from oracle import pyoracle as O
        return O.Oracle(self.prm, 1)

    def chain(self, images=None, tracking=True):
        images = self.eq if images is None else images
        if id(images) not in self._chains:
            orc, out = self.oracle(), []
            for pair in images:
                R, t = orc.track(*pair)
                out.append((np.array(R), np.array(t), orc.status, orc.counts()))
            self._chains[id(images)] = out
        out = self._chains[id(images)]
        if tracking:
            assert [r[2] for r in out] == [2] * len(out), "the oracle is not TRACKING on every frame: an early LOST would hide a difference"
        return out


_DIM = []


def dim_world():
    if not _DIM:
        _DIM.append(DimWorld())
    return _DIM[0]


def equalised_system(hip_lib, prm, tiles=TILES, clip=CLIP, sensor=1):
    hip = hip_lib.LvtSystem.create(prm, sensor)
    assert hip.set_equalisation(hip_lib.Equalisation(tiles, clip)) == 0, hip.last_error()
    e = hip.equalisation()
    assert e is not None and e.tiles == tuple(tiles) and np.float32(e.clip_limit) == np.float32(clip)
    return hip


def check_async(q, hip, got, ref, images):
    for i, (R, t, st) in enumerate(got):
        assert st == ref[i][2], f"frame {i}: state {st} oracle {ref[i][2]}"
        close_to(R, t, ref[i], f"frame {i}")
    orc = q.oracle()
    for pair in images[:len(got)]:
        orc.track(*pair)
    msgs = diff_frame(hip, orc)
    assert not msgs, msgs[:6]
    counts_equal(hip.counts(), ref[len(got) - 1][3], "last frame")


# ---- 2. the dimmed world through the GPU ---------------------------------------------------------------------------------------------------------
def test_the_dimmed_world_through_lvt_track(hip_lib, oracle_lib):
    """an equalised handle on the dimmed frames through lvt_track: TRACKING on all six and the complete frame diff against the oracle on the numpy-equalised
    frames is empty behind every frame; plane 5 is numpy's image and plane 6 numpy's tables, byte for byte, both eyes"""
    q = dim_world()
    ref = q.chain()
    hip, orc = equalised_system(hip_lib, q.prm), q.oracle()
    assert hip.plane(0, 5).size == 0                       # a set, but no frame yet
    for i in range(q.n):
        orc.track(*q.eq[i])
        R, t = hip.track(*q.dim[i])
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        assert hip.get_state() == orc.status == 2, i
        close_to(R, t, ref[i], f"frame {i}")
        if i in (0, q.n - 1):
            for eye in (0, 1):
                assert_plane(hip.plane(eye, 5), q.eq[i][eye], q.W, q.H, q.pitch, f"frame {i} eye {eye}")
                want = CL.luts(q.dim[i][eye], TILES, CLIP).reshape(-1, 256)
                assert np.array_equal(hip.plane(eye, 6), want), f"frame {i} eye {eye}: the tables differ"


def test_a_plain_handle_is_lost_where_the_oracle_is(hip_lib, oracle_lib):
    q = dim_world()
    ref = q.chain(q.dim, tracking=False)
    assert 3 in [r[2] for r in ref][:3], "the oracle is not LOST by frame 2 on the dimmed frames"
    hip = hip_lib.LvtSystem.create(q.prm, 1)
    for i in range(q.n):
        hip.track(*q.dim[i])
        assert hip.get_state() == ref[i][2], f"frame {i}: state {hip.get_state()} oracle {ref[i][2]}"
        counts_equal(hip.counts(), ref[i][3], f"frame {i}")
    assert hip.plane(0, 5).size == 0 and hip.equalisation() is None


# ---- 3. the other routes ---------------------------------------------------------------------------------------------------------------------
def test_equalised_frames_through_track_async(hip_lib, oracle_lib):
    """lvt_amd_track_async on host frames, three in flight"""
    q = dim_world()
    hip = equalised_system(hip_lib, q.prm)

    def submit(i):
        assert hip.track_async(*q.dim[i]) == 0, hip.last_error()
    got = run_async(hip, submit, q.n, 3)
    check_async(q, hip, got, q.chain(), q.eq)
    assert hip.host_stats()["async_host_frames"] == q.n


def test_equalised_device_planes_at_an_odd_pitch(hip_lib, oracle_lib):
    """planes in HBM at odd addresses with a pitch of W + 5 and 255 in every byte that is no pixel, three frames in flight, read in place"""
    q = dim_world()
    hip = equalised_system(hip_lib, q.prm)
    dev = [[device_colour(img[:, :, None], 1 + (i + eye) % 3) for eye, img in enumerate(q.dim[i])] for i in range(q.n)]
    assert dev[0][0][2] == q.W + 5

    def submit(i):
        hip.track_device_async(dev[i][0][1], dev[i][1][1], q.H, q.W, dev[i][0][2])
    got = run_async(hip, submit, q.n, 3)
    assert hip.last_error() == "", hip.last_error()
    check_async(q, hip, got, q.chain(), q.eq)
    for eye in (0, 1):
        assert_plane(hip.plane(eye, 5), q.eq[q.n - 1][eye], q.W, q.H, q.pitch, f"last frame eye {eye}")


def test_equalised_rgbd_frames(hip_lib, oracle_lib):
    """the tum world at 322 x 242, tiles 8 x 8: gray + 16-bit depth through lvt_amd_track_rgbd16, the oracle's track_rgbd on the numpy-equalised gray"""
    from oracle import pyoracle as O
    q = rgbd_seq()
    eq = [CL.clahe(g, (8, 8), 2.0) for g in q.raw_gray[:6]]
    hip, orc = equalised_system(hip_lib, q.prm, (8, 8), 2.0, sensor=2), O.Oracle(q.prm, 2)
    for i in range(6):
        Ro, to = orc.track_rgbd(eq[i], q.f32[i])
        R, t = hip.track(q.raw_gray[i], q.u16[i], depth_scale=SCALE)
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
    assert_plane(hip.plane(0, 5), eq[5], q.W, q.H, q.pitch, "last frame")


def test_colour_then_rectify_then_equalise(hip_lib, oracle_lib):
    """a BGR8 handle with rectifiers and an equalisation: plane 3 is the converted raw image, plane 2 the oracle's remap of that, plane 5 numpy's
    equalisation OF THAT; four frames against the oracle on those"""
    rc = raw_colour()
    c = rc.c
    eq = [tuple(CL.clahe(g, (4, 2), 4.0) for g in pair) for pair in rc.rect[:4]]
    hip = equalised_system(hip_lib, c.prm, (4, 2), 4.0)
    assert hip.set_pixel_format(CU.BGR8) == 0, hip.last_error()
    rl, rr = c.rectifiers(hip_lib)
    assert hip.set_rectifiers(rl, rr) == 0, hip.last_error()
    orc = c.oracle()
    for i in range(4):
        Ro, to = orc.track(*eq[i])
        R, t = hip.track(*rc.colour(i, CU.BGR8))
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        if i == 0:
            for eye in (0, 1):
                assert_plane(hip.plane(eye, 3), rc.gray[0][eye], c.W, c.H, c.pitch, f"converted, eye {eye}")
                assert_plane(hip.plane(eye, 2), rc.rect[0][eye], c.W, c.H, c.pitch, f"rectified, eye {eye}")
                assert_plane(hip.plane(eye, 5), eq[0][eye], c.W, c.H, c.pitch, f"equalised, eye {eye}")


def test_equalised_frames_with_external_corners(hip_lib, oracle_lib):
    """lvt_track_with_external_corners stays allowed: the corners -- the oracle's detector on the numpy-equalised frames -- are in the same coordinates, and
    the descriptors come from the equalised plane (features compared without the response)"""
    from oracle import pyoracle as O
    q = dim_world()
    hip, orc = equalised_system(hip_lib, q.prm), q.oracle()
    for i in range(4):
        cl = O.compute_features(q.eq[i][0], q.prm)[0].astype(np.float64)
        cr = O.compute_features(q.eq[i][1], q.prm)[0].astype(np.float64)
        Ro, to = orc.track_with_external_corners(q.eq[i][0], q.eq[i][1], cl, cr)
        R, t = hip.track_with_external_corners(*q.dim[i], cl, cr)
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"


def test_mixed_batch_of_equalised_plain_and_absent(hip_lib, oracle_lib):
    """three sequences of three image sizes in one chain, three steps in flight: 0 = the dimmed world, tiles 8 x 4; 1 = plain; 2 = tiles 4 x 2, clip 2, sitting
    out steps 2 and 4.  Each against its own oracle chain: state and pose of every step it has a frame in, all counters behind the last"""
    from oracle import pyoracle as O
    a, b, c = dim_world(), stereo_seq(32, (613, 185)), stereo_seq(71, (621, 187))
    gray_b = [tuple(np.ascontiguousarray(g) for g in b.world.render_stereo(i)) for i in range(6)]
    gray_c = [tuple(np.ascontiguousarray(g) for g in c.world.render_stereo(i)) for i in range(6)]
    eq_c = [tuple(CL.clahe(g, (4, 2), 2.0) for g in pair) for pair in gray_c]
    prms = [a.prm, b.prm, c.prm]
    batch = hip_lib.LvtBatch(prms)
    assert batch.set_equalisation(0, hip_lib.Equalisation(TILES, CLIP)) == 0 and batch.set_equalisation(2, tiles=(4, 2), clip_limit=2.0) == 0, batch.last_error()
    assert batch.equalisation(1) is None and batch.equalisation(0).tiles == TILES and batch.equalisation(2).tiles == (4, 2)
    nsteps = 6
    which = [[k, k, None] for k in range(nsteps)]
    f2 = 0
    for k in range(nsteps):
        if k not in (2, 4):
            which[k][2] = f2
            f2 += 1
    images = [a.eq, gray_b, eq_c]                          # what each sequence's oracle is given
    dev0 = [[device_colour(img[:, :, None], 1 + e) for e, img in enumerate(a.dim[i])] for i in range(nsteps)]
    dev1 = [device_gray([gray_b[i][e] for i in range(nsteps)], b.W, b.H, b.pitch) for e in (0, 1)]
    dev2 = [[device_colour(img[:, :, None], 3 - e, extra=0) for e, img in enumerate(gray_c[i])] for i in range(f2)]   # (tightly packed rows)

    def ptrs(s, i):
        if s == 1:
            return dev1[0][i].data_ptr(), dev1[1][i].data_ptr(), b.pitch
        d = (dev0, None, dev2)[s][i]
        return d[0][1], d[1][1], d[0][2]
    got, inflight = [], 0
    for k in range(nsteps):
        p = [None if which[k][s] is None else ptrs(s, which[k][s]) for s in range(3)]
        rc_ = batch.track_device_async_mixed([x and x[0] for x in p], [x and x[1] for x in p], [q.H for q in (a, b, c)], [q.W for q in (a, b, c)],
                                             [x[2] if x else 0 for x in p])
        assert rc_ == 0, batch.last_error()
        inflight += 1
        if inflight >= 3:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    assert batch.last_error() == "", batch.last_error()
    for s in range(3):
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


def test_set_then_unset(hip_lib, oracle_lib):
    """three equalised frames, collect, set_equalisation(None), three plain frames: ONE oracle chain covers all six, and plane 5 is empty again"""
    q = stereo_seq(71, (621, 187))
    gray = [tuple(np.ascontiguousarray(g) for g in q.world.render_stereo(i)) for i in range(6)]
    fed = [tuple(CL.clahe(g, (8, 8), 3.0) for g in gray[i]) if i < 3 else gray[i] for i in range(6)]
    hip, orc = equalised_system(hip_lib, q.prm, (8, 8), 3.0), q.oracle()
    for i in range(6):
        if i == 3:
            assert hip.set_equalisation(None) == 0, hip.last_error()
            assert hip.equalisation() is None
        Ro, to = orc.track(*fed[i])
        R, t = hip.track(*gray[i])
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(R, t, (np.array(Ro), np.array(to)), f"frame {i}")
        assert (hip.plane(0, 5).size != 0) == (i < 3)
    assert hip.set_equalisation(tiles=(8, 8), clip_limit=3.0) == 0
    assert hip.plane(0, 5).size == 0                       # the last frame went in before the record was set
    hip.track(*gray[5])
    assert hip.plane(0, 5).size != 0 and hip.plane(0, 6).shape == (64, 256)
    assert hip.set_equalisation(tiles=(4, 2), clip_limit=3.0) == 0
    assert hip.plane(0, 5).size == 0 and hip.plane(0, 6).size == 0   # ... before THIS record: another record's plane and tables are not handed out


# ---- 4. launches ---------------------------------------------------------------------------------------------------------------------------------
def _profile_of(h):
    return [(name, calls) for name, _ms, calls in h.profile_read()]


def test_launch_accounting(hip_lib, oracle_lib):
    """a handle that never set the property has neither row; an equalised handle reports exactly one k_clahe_lut and one k_clahe_apply call per frame and every
    other row as the plain handle"""
    q = dim_world()
    plain = hip_lib.LvtSystem.create(q.prm, 1)
    plain.profile_enable(True)
    for i in range(4):
        plain.track(*q.eq[i])
    rows = _profile_of(plain)
    assert rows and not [n for n, _ in rows if "clahe" in n], rows
    assert dict(rows)["k_score"] == 4
    plain.close()   # (a handle created beside a live one orders its streams with events: other rows)

    hip = equalised_system(hip_lib, q.prm)
    hip.profile_enable(True)
    for i in range(4):
        hip.track(*q.dim[i])
    prof = _profile_of(hip)
    assert dict(prof)["k_clahe_lut"] == 4 and dict(prof)["k_clahe_apply"] == 4, prof
    assert [(n, k) for n, k in prof if "clahe" not in n] == rows, (prof, rows)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_their_order(hip_lib, oracle_lib, tmp_path):
    """every refusal returns -1 with its sentence and "(nothing was changed)"; where two objections apply the earlier one of the contract's order is named:
    the handle's kind, the spelling, the sequence, the record, frames in flight; and the handle then tracks its next plain frame as the oracle does"""
    q = stereo_seq(71, (621, 187))
    gray = [tuple(np.ascontiguousarray(g) for g in q.world.render_stereo(i)) for i in range(3)]
    L, E, C = hip_lib.load_library(), hip_lib.Equalisation, hip_lib.C
    good = E((8, 8), 3.0)
    hip, orc = hip_lib.LvtSystem.create(q.prm, 1), q.oracle()
    said = []

    def refused(h, rc, *words):
        err = h.last_error()
        assert rc == -1 and err.endswith("(nothing was changed)") and all(w in err for w in words), (rc, err, words)
        said.append(err)

    assert L.lvt_amd_get_plane(hip._h, 0, 5, None, 0, None) == 0      # 0 bytes before a set
    for tiles, word in (((0, 8), "tiles_x = 0 (1 ... 16)"), ((17, 8), "tiles_x = 17 (1 ... 16)"), ((8, 0), "tiles_y = 0 (1 ... 16)"), ((8, 17), "tiles_y = 17 (1 ... 16)")):
        refused(hip, hip.set_equalisation(E(tiles, 3.0)), word)
    for clip in (float("nan"), float("inf"), 0.0, -2.0):
        refused(hip, hip.set_equalisation(E((8, 8), clip)), "clip_limit is not finite and > 0")
    refused(hip, L.lvt_amd_batch_set_equalisation(hip._h, 0, C.byref(good)), "lvt_amd_batch_set_equalisation on a handle that is not a batch")
    refused(hip, L.lvt_amd_batch_set_equalisation(hip._h, 5, C.byref(E((0, 0), 0.0))), "not a batch")          # the spelling before the sequence and the record
    assert hip.equalisation() is None
    dev = device_gray([gray[0][0], gray[0][1]], q.W, q.H, q.pitch)
    hip.track_device_async(dev[0].data_ptr(), dev[1].data_ptr(), q.H, q.W, q.pitch)
    refused(hip, hip.set_equalisation(good), "frames in flight")
    refused(hip, hip.set_equalisation(E((17, 8), 3.0)), "tiles_x = 17")                                         # the record before the frames in flight
    R, t, st = hip.wait_status()
    orc.track(*gray[0])
    assert st == orc.status
    Ro, to = orc.track(*gray[1])
    R, t = hip.track(*gray[1])
    msgs = [m for m in diff_frame(hip, orc) if m != "hip error: " + said[-1]]
    assert not msgs, msgs[:6]
    assert hip.plane(0, 5).size == 0 and hip.equalisation() is None

    seat = hip_lib.LvtSystem.create(q.prm, 1, pooled=True)
    refused(seat, seat.set_equalisation(good), "a pooled handle")
    refused(seat, seat.set_equalisation(E((0, 8), 3.0)), "a pooled handle")                                     # the kind before the record
    assert seat.equalisation() is None
    q.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    autos = [hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1) for _ in range(2)]
    assert autos[0].ordering() == "pooled"
    refused(autos[0], autos[0].set_equalisation(good), "a pooled handle")
    seat.close()
    for h in autos:
        h.close()

    batch = hip_lib.LvtBatch(q.prm, 2)
    for seq in (-1, 2):
        refused(batch, batch.set_equalisation(seq, good), f"no sequence {seq}")
        with pytest.raises(IndexError):
            batch.equalisation(seq)
    refused(batch, batch.set_equalisation(2, E((0, 8), 3.0)), "no sequence 2")                                  # the sequence before the record
    refused(batch, L.lvt_amd_set_equalisation(batch._h, C.byref(good)), "a batch handle takes its equalisation per sequence")
    refused(batch, batch.set_equalisation(1, E((8, 8), -1.0)), "clip_limit")
    assert L.lvt_amd_get_equalisation(None, 0, None) == -1
    assert batch.set_equalisation(1, good) == 0 and batch.equalisation(1).tiles == (8, 8) and batch.equalisation(0) is None
    assert batch.set_equalisation(1, None) == 0 and batch.equalisation(1) is None


def test_a_set_is_a_use_of_an_lvt_create_handle(hip_lib, oracle_lib, tmp_path):
    """lvt_create, set_equalisation, a second lvt_create with the same parameters: the first handle keeps its own chain, and equalises"""
    q = dim_world()
    q.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    first = hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1)
    assert first.set_equalisation(tiles=TILES, clip_limit=CLIP) == 0, first.last_error()
    second = hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1)
    assert first.ordering() != "pooled"
    first.track(*q.dim[0])
    assert_plane(first.plane(0, 5), q.eq[0][0], q.W, q.H, q.pitch, "eye 0")
    second.close(); first.close()


# ---- 6. snapshots --------------------------------------------------------------------------------------------------------------------------------
def test_snapshot_bytes_do_not_know_the_property(hip_lib, oracle_lib):
    """four dimmed frames through an equalised handle, the same frames equalised by numpy through a plain handle: the exported snapshots are the same bytes;
    reset leaves the record in place"""
    q = dim_world()
    hip, plain = equalised_system(hip_lib, q.prm), hip_lib.LvtSystem.create(q.prm, 1)
    for i in range(4):
        hip.track(*q.dim[i])
        plain.track(*q.eq[i])
    assert hip.get_state() == plain.get_state() == 2
    a, b = hip.snapshot().to_bytes(), plain.snapshot().to_bytes()
    assert a == b, "the snapshot of an equalised handle differs from the plain handle's on the same equalised frames"
    hip.reset()
    assert hip.equalisation().tiles == TILES
    hip.track(*q.dim[0])
    assert_plane(hip.plane(0, 5), q.eq[0][0], q.W, q.H, q.pitch, "after reset, eye 0")
