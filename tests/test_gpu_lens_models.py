"""LENS MODELS on the GPU: rectifiers of lvt_amd_rectifier_create_lens (twelve-coefficient RADTAN, FISHEYE), a raw image whose size is not the rectified
one's, and raw frames of that size through every stereo entry point of a tracker ("LENS MODELS" and "RAW stereo frames", include/lvt_amd_ext.h).

The maps are held to the numpy restatement (tests/lens_util.py); the planes to remap_util.remap under the maps the LIBRARY reports; the sequences to the
oracle fed that remap of the raw frames (tests/lens_cases.py: the worlds tests/test_lens_models.py shows the oracle can track).  Every expected value is
computed once per case and shared."""
import ctypes as C
import math

import numpy as np
import pytest

import lens_util as LU
from lens_util import RADTAN, FISHEYE
from lens_cases import get_case, EYE3, RADTAN12, N_FRAMES
from parity_util import make_case, diff_frame, pose_errors, POSE_TOL
from remap_util import remap, rectify_maps, maps_equal, to_fixed

pytestmark = pytest.mark.gpu

EUROC_K = [458.654, 0.0, 367.215, 0.0, 457.296, 248.375, 0.0, 0.0, 1.0]
EUROC_R = [0.999966347530033, -0.001422739138722922, 0.008079580483432283, 0.001365741834644127, 0.9999741760894847,
           0.007055629199258132, -0.008089410156878961, -0.007044357138835809, 0.9999424675829176]
EUROC_P_HALF = [217.60234798572995, 0.0, 183.7258605957031, 0.0, 217.60234798572995, 126.10042572021485, 0.0, 0.0, 1.0]
_A75 = math.radians(75.0)
ROT_Y_75 = [math.cos(_A75), 0.0, math.sin(_A75), 0.0, 1.0, 0.0, -math.sin(_A75), 0.0, math.cos(_A75)]
K_HORIZON = [30.0, 0.0, 33.2, 0.0, 30.0, 17.4, 0.0, 0.0, 1.0]
# (source, destination, K, R, P): a destination width of 3 mod 4; a source smaller than the destination; EuRoC cam0 to half size
SHAPES = {
    "90x50_to_67x35": ((90, 50), (67, 35), [60.0, 0.0, 44.3, 0.0, 61.0, 24.6, 0.0, 0.0, 1.0], EYE3, [45.0, 0.0, 33.1, 0.0, 45.0, 17.2, 0.0, 0.0, 1.0]),
    "33x40_to_64x64": ((33, 40), (64, 64), [25.0, 0.0, 16.2, 0.0, 26.0, 19.7, 0.0, 0.0, 1.0], EYE3, [48.0, 0.0, 31.6, 0.0, 48.0, 32.3, 0.0, 0.0, 1.0]),
    "752x480_to_376x240": ((752, 480), (376, 240), EUROC_K, EUROC_R, EUROC_P_HALF),
    "horizon_67x35": ((67, 35), (67, 35), K_HORIZON, ROT_Y_75, K_HORIZON),
}
FISHEYE_D = {"90x50_to_67x35": [0.6, 0.05, 0.0, 0.0], "33x40_to_64x64": [-0.02, 0.004, -0.001, 0.0002], "752x480_to_376x240": [-0.013, 0.02, -0.012, 0.002],
             "horizon_67x35": [0.0, 0.0, 0.0, 0.0]}
PINCUSHION = [0.12, 0.02, 2e-4, -1e-4, 0.0]


def _rectifier(hip_lib, model, shape, D):
    (sw, sh), (dw, dh), K, R, P = SHAPES[shape]
    return hip_lib.Rectifier.from_lens(hip_lib.Lens(model, sw, sh, K, D), R, P, dw, dh)


# ---- 1. the maps ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["90x50_to_67x35", "33x40_to_64x64", "752x480_to_376x240"])
def test_radtan_maps_equal_numpy_bit_for_bit(hip_lib, shape):
    (sw, sh), (dw, dh), K, R, P = SHAPES[shape]
    r = _rectifier(hip_lib, RADTAN, shape, RADTAN12)
    m1, m2 = r.maps()
    assert m1.shape == (dh, dw) and m2.shape == (dh, dw)
    w1, w2 = LU.lens_maps(RADTAN, K, RADTAN12, R, P, dw, dh)
    for got, want, which in ((m1, w1, "map1"), (m2, w2, "map2")):
        bad = np.argwhere(~((np.isnan(got) & np.isnan(want)) | (got.view(np.uint32) == want.view(np.uint32))))
        assert len(bad) == 0, f"{shape} {which}: {len(bad)} entries differ, first at {tuple(bad[0])}: hip {got[tuple(bad[0])]!r} numpy {want[tuple(bad[0])]!r}"


def test_radtan_with_seven_zeros_equals_the_old_call(hip_lib):
    """RADTAN with k4 ... s4 = 0 and equal sizes: bit for bit lvt_amd_rectifier_create's maps (and numpy's plumb-bob restatement)"""
    from test_oracle_primitives import EUROC_L as c
    old = hip_lib.Rectifier(c["K"], c["D"], c["R"], c["P"], 752, 480)
    new = hip_lib.Rectifier.from_lens(hip_lib.Lens(RADTAN, 752, 480, c["K"], list(c["D"]) + [0.0] * 7), c["R"], c["P"], 752, 480)
    (o1, o2), (n1, n2) = old.maps(), new.maps()
    assert maps_equal(n1, o1) and maps_equal(n2, o2)
    w1, w2 = rectify_maps(c["K"], c["D"], c["R"], c["P"], 752, 480)
    assert maps_equal(o1, w1) and maps_equal(o2, w2)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fisheye_maps_equal_numpy_up_to_atans_last_bit(hip_lib, shape):
    """atan is the one operation whose last bit the device library and libm may not share.  The condition: the +-inf entries and their signs identical; every
    other entry within 1 fp32 ulp; at most 1e-5 of the entries differ at all (a few fp64 ulp in atan move an fp32 rounding with probability about 2^-26
    per entry: the cap is a thousand times that); no fixed-point entry differs by more than 1.  The count observed is printed (profiles/lens_models.md)."""
    (sw, sh), (dw, dh), K, R, P = SHAPES[shape]
    D = FISHEYE_D[shape]
    m = _rectifier(hip_lib, FISHEYE, shape, D).maps()
    w = LU.lens_maps(FISHEYE, K, D, R, P, dw, dh)
    n_diff = 0
    for got, want, which in ((m[0], w[0], "map1"), (m[1], w[1], "map2")):
        assert got.shape == (dh, dw)
        assert np.array_equal(np.isinf(got), np.isinf(want)), f"{shape} {which}: the sets of infinite entries differ"
        inf = np.isinf(want)
        assert np.array_equal(np.signbit(got[inf]), np.signbit(want[inf])), f"{shape} {which}: an infinite entry's sign differs"
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{shape} {which}: the sets of NaN entries differ"
        fin = np.isfinite(want)
        ulp = LU.ulp_distance(got[fin], want[fin])
        n_diff += int(np.count_nonzero(ulp))
        assert ulp.max(initial=0) <= 1, f"{shape} {which}: an entry is {int(ulp.max())} fp32 ulp from numpy's"
        fx = np.abs(to_fixed(got) - to_fixed(want))
        assert fx.max() <= 1, f"{shape} {which}: a fixed-point entry differs by {int(fx.max())}"
    n_inf = int(np.count_nonzero(np.isinf(w[0])))
    print(f"fisheye maps {shape}: {n_diff} of {2 * dw * dh} entries differ from numpy's; {n_inf} of {dw * dh} pixels are +-inf")
    assert n_diff <= 1e-5 * 2 * dw * dh
    if shape == "horizon_67x35":
        assert n_inf == 910      # (a condition on the input: the _w <= 0 branch runs)
        r = _rectifier(hip_lib, FISHEYE, shape, D)
        out = r.rectify(np.full((sh, sw), 200, np.uint8))
        assert not out[np.isinf(w[0])].any(), "a pixel behind the camera is not 0"


# ---- 2. the planes --------------------------------------------------------------------------------------------------------------------------------
PLANE_CASES = ["fisheye_strong", "fisheye_small", "radtan12", "radtan_small"]


def _expected_plane(c, rect, eye, pitch=None):
    m1, m2 = rect.maps()
    return remap(c.raw[0][eye], m1, m2, out_pitch=pitch)[0]


def _device_u8(a, pitch, pad=255):
    import torch
    t = torch.full((a.shape[0], pitch), pad, dtype=torch.uint8, device="cuda")
    t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("name", PLANE_CASES)
def test_rectify_host_and_device_equal_the_numpy_remap(hip_lib, name):
    """lvt_amd_rectify on a tightly packed source of the lens's size, and lvt_amd_rectify_device at a source pitch that is not its width: byte for byte
    remap_util.remap under the library's own maps, the destination's padding columns zero"""
    import torch
    c = get_case(name)
    r = c.rectifier(hip_lib)
    assert (r.src_w, r.src_h, r.w, r.h) == (c.sw, c.sh, c.dw, c.dh)
    want = _expected_plane(c, r, 0)
    got = r.rectify(c.raw[0][0])
    assert got.shape == (c.dh, c.dw) and np.array_equal(got, want), f"{name}: {np.count_nonzero(got != want)} pixels differ (lvt_amd_rectify)"
    spitch, dpitch = c.sw + 5, c.pitch + 4
    src = _device_u8(c.raw[0][0], spitch)
    dst = torch.full((c.dh, dpitch), 7, dtype=torch.uint8, device="cuda")
    assert r.rectify_device(src.data_ptr(), spitch, dst.data_ptr(), dpitch) == 0
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert np.array_equal(out[:, :c.dw], want) and not out[:, c.dw:].any(), f"{name}: lvt_amd_rectify_device"
    assert r.rectify_device(src.data_ptr(), c.sw - 1, dst.data_ptr(), dpitch) == -1      # (a source pitch under the lens's width)
    with pytest.raises(ValueError):
        r.rectify(np.zeros((c.dh, c.dw), np.uint8))      # (an image of the DESTINATION's size is no source)


def _attached(hip_lib, c):
    hip = hip_lib.LvtSystem.create(c.prm, 1)
    r = c.rectifier(hip_lib)
    assert hip.set_rectifiers(r, r) == 0, hip.last_error()
    hip._lens_rect = r      # (borrowed by the handle: kept alive with it)
    return hip


@pytest.mark.parametrize("route", ["lvt_track", "track_device"])
@pytest.mark.parametrize("name", PLANE_CASES)
def test_rectified_plane_of_an_attached_handle(hip_lib, oracle_lib, name, route):
    """after one raw frame of the SOURCE's size, plane(eye, 2) is remap_util.remap(raw, the library's maps) at the handle's pitch, padding columns zero"""
    c = get_case(name)
    hip = _attached(hip_lib, c)
    if route == "lvt_track":
        hip.track(*c.raw[0])
    else:
        import torch
        spitch = c.sw + 3
        dl, dr = _device_u8(c.raw[0][0], spitch), _device_u8(c.raw[0][1], spitch)
        hip.track_device(dl.data_ptr(), dr.data_ptr(), c.sh, c.sw, spitch)
    assert hip.last_error() == "", hip.last_error()
    for eye in (0, 1):
        p = hip.plane(eye, 2)
        assert p.shape == (c.dh, c.pitch)
        want = _expected_plane(c, hip._lens_rect, eye, c.pitch)
        bad = np.argwhere(p != want)
        assert len(bad) == 0, f"{name} eye {eye}: {len(bad)} bytes differ, first at {tuple(bad[0])}"


# ---- 3. sequences ---------------------------------------------------------------------------------------------------------------------------------
_CHAINS = {}


def _library_rect(hip_lib, c, key="library", pre=None, post=None):
    """the raw frames (through `pre`, e.g. a colour conversion) remapped by numpy under the maps the LIBRARY built (then through `post`, e.g. CLAHE)"""
    if key not in c._rect:
        m1, m2 = c.rectifier(hip_lib).maps()
        f = (lambda x: x) if post is None else post
        g = (lambda x, i, e: x) if pre is None else pre
        c._rect[key] = [(f(remap(g(a, i, 0), m1, m2)[0]), f(remap(g(b, i, 1), m1, m2)[0])) for i, (a, b) in enumerate(c.raw)]
    return c._rect[key]


def _chain(oracle_lib, c, frames, key):
    """[(R, t, state, counts)] of the oracle over `frames`"""
    if (c.name, key) not in _CHAINS:
        orc, out = oracle_lib.Oracle(c.prm, 1), []
        for L, R in frames:
            Ro, to = orc.track(L, R)
            out.append((np.array(Ro), np.array(to), orc.status, orc.counts()))
        assert [r[2] for r in out] == [2] * len(out), f"{c.name}: the oracle is not TRACKING on every frame: an early LOST would hide a difference"
        _CHAINS[(c.name, key)] = out
    return _CHAINS[(c.name, key)]


def _close_to(R, t, ref, what):
    e_t, e_R = pose_errors(np.asarray(R), np.asarray(t), ref[0], ref[1])
    assert e_t <= POSE_TOL and e_R <= POSE_TOL, f"{what}: e_t {e_t:.2e} e_R {e_R:.2e}"


def _counts_equal(ch, co, what):
    bad = {k: (ch.get(k), v) for k, v in co.items() if ch.get(k) != v}
    assert not bad, f"{what}: counters (hip, oracle) {bad}"


def _sync_sequence(hip_lib, oracle_lib, c, hip, raw, frames):
    orc = oracle_lib.Oracle(c.prm, 1)
    for i in range(N_FRAMES):
        Ro, to = orc.track(*frames[i])
        R, t = hip.track(*raw[i])
        assert hip.last_error() == "", hip.last_error()
        msgs = diff_frame(hip, orc)
        assert not msgs, (c.name, i, msgs[:6])
        _close_to(R, t, (np.array(Ro), np.array(to)), f"{c.name} frame {i}")
    assert orc.status == 2


@pytest.mark.parametrize("name", ["fisheye_strong", "fisheye_mild", "radtan12"])
def test_raw_sequence_through_lvt_track(hip_lib, oracle_lib, name):
    """8 raw frames of the source's size through lvt_track: the complete frame diff against the oracle is empty on every frame"""
    c = get_case(name)
    frames = _library_rect(hip_lib, c)
    _chain(oracle_lib, c, frames, "library")
    _sync_sequence(hip_lib, oracle_lib, c, _attached(hip_lib, c), c.raw, frames)


def test_colour_raw_sequence_converts_at_the_source_size_then_remaps(hip_lib, oracle_lib):
    """fisheye_small with a BGR pixel format: the conversion runs at the SOURCE's size (plane 3 has the source's rows), the remap behind it"""
    import colour_util as CU
    c = get_case("fisheye_small")
    col = [tuple(CU.colourise(g, CU.BGR8, 71, i, e) for e, g in enumerate(pair)) for i, pair in enumerate(c.raw)]
    frames = _library_rect(hip_lib, c, "colour", pre=lambda g, i, e: CU.to_gray(col[i][e], CU.BGR8))
    _chain(oracle_lib, c, frames, "colour")
    hip = hip_lib.LvtSystem.create(c.prm, 1)
    assert hip.set_pixel_format(CU.BGR8) == 0, hip.last_error()       # (the format first, the rectifiers second: the converted planes follow the attach)
    r = c.rectifier(hip_lib)
    assert hip.set_rectifiers(r, r) == 0, hip.last_error()
    _sync_sequence(hip_lib, oracle_lib, c, hip, col, frames)
    g = hip.plane(0, 3)
    assert g.shape[0] == c.sh and g.shape[1] >= c.sw
    assert np.array_equal(g[:, :c.sw], CU.to_gray(col[N_FRAMES - 1][0], CU.BGR8)) and not g[:, c.sw:].any()


def test_colour_format_set_behind_the_attach(hip_lib, oracle_lib):
    """the other order on a LARGER source -- rectifiers first, then RGBA: the same planes, the same answer, three frames"""
    import colour_util as CU
    c = get_case("fisheye_mild")
    col = [tuple(CU.colourise(g, CU.RGBA8, 71, i, e) for e, g in enumerate(pair)) for i, pair in enumerate(c.raw[:3])]
    m1, m2 = c.rectifier(hip_lib).maps()
    hip = _attached(hip_lib, c)
    assert hip.set_pixel_format(CU.RGBA8) == 0, hip.last_error()
    orc = oracle_lib.Oracle(c.prm, 1)
    for i in range(3):
        orc.track(*(remap(CU.to_gray(col[i][e], CU.RGBA8), m1, m2)[0] for e in (0, 1)))
        hip.track(*col[i])
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
    assert orc.status == 2


def _run_async(hip, submit, n, depth):
    got, inflight = [], 0
    for i in range(n):
        submit(i)
        inflight += 1
        if inflight >= depth:
            got.append(hip.wait_status()); inflight -= 1
    while inflight:
        got.append(hip.wait_status()); inflight -= 1
    return got


def _async_checks(oracle_lib, c, hip, got, frames, key):
    ref = _chain(oracle_lib, c, frames, key)
    for i, (R, t, st) in enumerate(got):
        assert st == ref[i][2], f"{c.name} frame {i}: state {st} oracle {ref[i][2]}"
        _close_to(R, t, ref[i], f"{c.name} frame {i}")
    orc = oracle_lib.Oracle(c.prm, 1)
    for L, R in frames:
        orc.track(L, R)
    msgs = diff_frame(hip, orc)
    assert not msgs, msgs[:6]
    _counts_equal(hip.counts(), ref[-1][3], "last frame")


def _pinned(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy()


@pytest.mark.parametrize("memory", ["pageable", "page_locked"])
@pytest.mark.parametrize("name", ["fisheye_strong", "fisheye_mild", "radtan12"])
def test_raw_frames_through_track_async(hip_lib, oracle_lib, name, memory):
    """lvt_amd_track_async on raw host frames of the source's size, three in flight: the staging, the image ring and the pull fused into the previous
    frame's corner-cell launch carry source-sized planes"""
    c = get_case(name)
    frames = _library_rect(hip_lib, c)
    hip = _attached(hip_lib, c)
    bufs = [(_pinned(a), _pinned(b)) if memory == "page_locked" else (a, b) for a, b in c.raw]

    def submit(i):
        assert hip.track_async(bufs[i][0], bufs[i][1]) == 0, hip.last_error()
    got = _run_async(hip, submit, N_FRAMES, 3)
    assert hip.last_error() == "", hip.last_error()
    _async_checks(oracle_lib, c, hip, got, frames, "library")
    hs = hip.host_stats()
    assert hs["async_host_frames"] == N_FRAMES and (hs["planes_in_place"] if memory == "page_locked" else hs["planes_staged"]) == 2 * N_FRAMES, hs


def _device_frames(raw, W, H, pitch, pad=255):
    import torch
    t = torch.full((len(raw), 2, H, pitch), pad, dtype=torch.uint8, device="cuda")
    for i, (a, b) in enumerate(raw):
        t[i, 0, :, :W] = torch.from_numpy(a).cuda(); t[i, 1, :, :W] = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("name", ["fisheye_strong", "fisheye_mild", "radtan12"])
def test_raw_frames_through_track_device_async(hip_lib, oracle_lib, name):
    """raw planes in HBM at the source's size with a pitch of their own, three frames in flight, read in place.  radtan12 runs with an equalisation set as
    well: the remap at the source's size, CLAHE behind it at the sequence's"""
    import clahe_util
    c = get_case(name)
    eq = name == "radtan12"
    key = "equalised" if eq else "library"
    frames = _library_rect(hip_lib, c, key, post=(lambda x: clahe_util.clahe(x[:, :c.dw], (8, 8), 3.0)) if eq else None)
    hip = _attached(hip_lib, c)
    if eq:
        assert hip.set_equalisation(tiles=(8, 8), clip_limit=3.0) == 0, hip.last_error()
    pitch = c.sw + 7
    dev = _device_frames(c.raw, c.sw, c.sh, pitch)
    got = _run_async(hip, lambda i: hip.track_device_async(dev[i, 0].data_ptr(), dev[i, 1].data_ptr(), c.sh, c.sw, pitch), N_FRAMES, 3)
    assert hip.last_error() == "", hip.last_error()
    _async_checks(oracle_lib, c, hip, got, frames, key)


def _old_style_case():
    """the kitti world 71 at 621 x 187 under a five-coefficient pincushion rectifier of lvt_amd_rectifier_create (source = destination)"""
    world, prm, _ = make_case("kitti", 71, size=(621, 187))
    K = [world.fx, 0.0, world.cx, 0.0, world.fy, world.cy, 0.0, 0.0, 1.0]
    raw = [tuple(np.ascontiguousarray(x) for x in world.render_stereo(i)) for i in range(N_FRAMES)]
    return world, prm, K, raw


def test_mixed_batch_fisheye_old_style_plain_and_a_sit_out(hip_lib, oracle_lib):
    """a mixed batch of four over 8 steps, three in flight: 0 = fisheye_strong (a LARGER source), 1 = an old-style rectifier sequence, 2 = a plain sequence,
    3 = radtan12, present for steps 0 - 4 and sitting out afterwards.  Every sequence against its own oracle chain"""
    cf, cr = get_case("fisheye_strong"), get_case("radtan12")
    world, prm, K, raw = _old_style_case()
    old = hip_lib.Rectifier(K, PINCUSHION, EYE3, K, 621, 187)
    om1, om2 = old.maps()
    old_frames = [(remap(a, om1, om2)[0], remap(b, om1, om2)[0]) for a, b in raw]

    class _Plain:
        name = "old_style_world"
    _Plain.prm = prm
    refs = [_chain(oracle_lib, cf, _library_rect(hip_lib, cf), "library"), _chain(oracle_lib, _Plain, old_frames, "old_style"),
            _chain(oracle_lib, _Plain, raw, "plain"), _chain(oracle_lib, cr, _library_rect(hip_lib, cr), "library")]
    batch = hip_lib.LvtBatch([cf.prm, prm, prm, cr.prm])
    rf, rr = cf.rectifier(hip_lib), cr.rectifier(hip_lib)
    assert batch.set_rectifiers(0, rf, rf) == 0 and batch.set_rectifiers(1, old, old) == 0 and batch.set_rectifiers(3, rr, rr) == 0, batch.last_error()
    sizes = [(cf.sw, cf.sh), (621, 187), (621, 187), (cr.sw, cr.sh)]
    pitches = [cf.sw + 1, 621, 640, cr.sw]      # (raw planes: any pitch that holds a row; the plain sequence keeps the pitch % 16 rule)
    devs = [_device_frames(f, w, h, p, pad=(0 if s == 2 else 255)) for s, (f, (w, h), p) in enumerate(zip([cf.raw, raw, raw, cr.raw], sizes, pitches))]
    # the tracker's own size on the sequence whose source is larger: refused, nothing enqueued
    lp, rp = [d[0, 0].data_ptr() for d in devs], [d[0, 1].data_ptr() for d in devs]
    assert batch.track_device_async_mixed(lp, rp, [cf.dh, 187, 187, cr.sh], [cf.dw, 621, 621, cr.sw], pitches) == -1
    assert "sequence 0" in batch.last_error(), batch.last_error()
    got = []
    inflight = 0
    for k in range(N_FRAMES):
        here = [True, True, True, k < 5]
        lp = [devs[s][k, 0].data_ptr() if here[s] else None for s in range(4)]
        rp = [devs[s][k, 1].data_ptr() if here[s] else None for s in range(4)]
        assert batch.track_device_async_mixed(lp, rp, [h for _, h in sizes], [w for w, _ in sizes], pitches) == 0, batch.last_error()
        inflight += 1
        if inflight >= 3:
            got.append(batch.wait()); inflight -= 1
    while inflight:
        got.append(batch.wait()); inflight -= 1
    for s in range(4):
        for k in range(N_FRAMES):
            ref = refs[s][min(k, 4) if s == 3 else k]
            R, t, st = got[k]
            assert st[s] == ref[2], f"sequence {s} step {k}: state {st[s]} oracle {ref[2]}"
            _close_to(R[s], t[s], ref, f"sequence {s} step {k}")
        _counts_equal(batch.counts(s), refs[s][4 if s == 3 else -1][3], f"sequence {s} after the last step")


# ---- 4. launch accounting -------------------------------------------------------------------------------------------------------------------------
def _profile_of(h):
    return [(name, calls) for name, _ms, calls in h.profile_read()]


def test_launch_accounting(hip_lib, oracle_lib):
    """an attached handle of either model launches what a handle with old-style rectifiers launches -- one k_rectify_frames per step, nothing else new --,
    and a never-attached handle has no such slot"""
    world, prm, K, raw = _old_style_case()

    def profile(attach, frames):
        hip = hip_lib.LvtSystem.create(prm, 1)
        keep = attach(hip)
        hip.profile_enable(True)
        for i in range(4):
            hip.track(*frames[i])
        assert hip.last_error() == "", hip.last_error()
        out = _profile_of(hip)
        hip.close()
        del keep
        return out
    plain = profile(lambda hip: None, raw)
    assert plain and not [n for n, _ in plain if "k_rectify_frames" in n], plain

    def old_style(hip):
        r = hip_lib.Rectifier(K, PINCUSHION, EYE3, K, 621, 187)
        assert hip.set_rectifiers(r, r) == 0, hip.last_error()
        return r
    old = profile(old_style, raw)
    assert dict(old)["k_rectify_frames"] == 4 and [(n, k) for n, k in old if n != "k_rectify_frames"] == plain, (old, plain)
    for name in ("fisheye_strong", "fisheye_small"):
        c = get_case(name)
        assert (c.dw, c.dh) == (621, 187)

        def lens(hip, c=c):
            r = c.rectifier(hip_lib)
            assert hip.set_rectifiers(r, r) == 0, hip.last_error()
            return r
        assert profile(lens, c.raw) == old, name
    c = get_case("radtan12")
    hip = _attached(hip_lib, c)
    hip.profile_enable(True)
    for i in range(4):
        hip.track(*c.raw[i])
    prof = _profile_of(hip)
    assert dict(prof)["k_rectify_frames"] == 4 and [n for n, _ in prof] == [n for n, _ in old], prof


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refused_lens_records_in_the_contracts_order(hip_lib):
    """lvt_amd_rectifier_create_lens returns NULL with the sentence in lvt_amd_last_error(NULL): a NULL argument; an unknown model; a source side outside
    1 ... 8192; a destination side outside 1 ... 8192; a non-finite field of K or D; a non-finite field of R or Pnew -- an input that breaks two rules is
    told the first"""
    L = hip_lib.load_library()
    K = [60.0, 0.0, 44.3, 0.0, 61.0, 24.6, 0.0, 0.0, 1.0]
    nine = (C.c_double * 9)(*EYE3)
    rec = hip_lib.Lens(FISHEYE, 90, 50, K, [0.1])._record()
    for args in ((None, nine, nine), (C.byref(rec), None, nine), (C.byref(rec), nine, None)):
        assert not L.lvt_amd_rectifier_create_lens(args[0], args[1], args[2], 67, 35)
        assert "NULL argument" in hip_lib.last_call_error() and hip_lib.last_call_error().endswith("(nothing was created)")

    def refused(word, model=FISHEYE, sw=90, sh=50, K=K, D=(0.1,), R=EYE3, P=EYE3, dw=67, dh=35):
        with pytest.raises(ValueError) as e:
            hip_lib.Rectifier.from_lens(hip_lib.Lens(model, sw, sh, K, D), R, P, dw, dh)
        msg = str(e.value)
        assert msg.startswith("lvt_amd_rectifier_create_lens: ") and word in msg and msg.endswith("(nothing was created)"), msg
    nanK = list(K); nanK[4] = float("nan")
    infR = list(EYE3); infR[2] = float("inf")
    nanP = list(EYE3); nanP[8] = float("nan")
    refused("unknown lens model 2", model=2)
    refused("unknown lens model -1", model=-1, sw=0)                      # (the model before the size)
    for sw, sh in ((0, 50), (90, 0), (8193, 50), (90, 8193), (-4, 50)):
        refused("a source of", sw=sw, sh=sh, dw=0)                        # (the source before the destination)
    for dw, dh in ((0, 35), (67, 0), (8193, 35), (67, 8193)):
        refused("a destination of", dw=dw, dh=dh, K=nanK)                 # (the destination before the fields)
    refused("non-finite field of K or D", K=nanK, R=infR)                 # (the lens before R and Pnew)
    refused("non-finite field of K or D", D=[0.1, float("inf")])
    refused("non-finite field of K or D", model=RADTAN, D=[0.0] * 11 + [float("nan")])
    refused("non-finite field of R or Pnew", R=infR)
    refused("non-finite field of R or Pnew", P=nanP)
    # FISHEYE reads D[0 ... 3] only: what lies behind them is ignored, and reads back as zero
    r = hip_lib.Rectifier.from_lens(hip_lib.Lens(FISHEYE, 90, 50, K, [0.1, 0.0, 0.0, 0.0, float("nan"), 5.0]), EYE3, EYE3, 67, 35)
    assert list(r.info()[0].D[4:]) == [0.0] * 8
    # the limits themselves are accepted
    hip_lib.Rectifier.from_lens(hip_lib.Lens(RADTAN, 8192, 1, K, []), EYE3, EYE3, 1, 1)
    hip_lib.Rectifier.from_lens(hip_lib.Lens(RADTAN, 1, 1, K, []), EYE3, EYE3, 1, 8192)


def test_refused_attachments_and_frames_of_the_wrong_size(hip_lib, oracle_lib):
    """set_rectifiers: a destination that is not the sequence's size; two source sizes (the sentence names both); frames in flight.  Frames: with rectifiers
    whose source is not the tracker's size attached, every stereo entry point refuses the tracker's own size.  Each refusal leaves the handle as it was and the
    frames in flight untouched"""
    c, small, other = get_case("fisheye_strong"), get_case("fisheye_small"), get_case("radtan12")
    frames = _library_rect(hip_lib, c)
    ref = _chain(oracle_lib, c, frames, "library")
    r, r_small, r_other = c.rectifier(hip_lib), small.rectifier(hip_lib), other.rectifier(hip_lib)

    def refused(h, rc, *words):
        assert rc == -1 and all(w in h.last_error() for w in words), (rc, h.last_error())

    hip = hip_lib.LvtSystem.create(c.prm, 1)
    refused(hip, hip.set_rectifiers(r_other, r_other), "613 x 185", "621 x 187", "(nothing was changed)")       # the DESTINATION is not the sequence's
    refused(hip, hip.set_rectifiers(r_other, r_small), "613 x 185")                                              # (the destination before the sources)
    refused(hip, hip.set_rectifiers(r, r_small), "828 x 250", "500 x 150", "(nothing was changed)")              # two source sizes
    refused(hip, hip.set_rectifiers(r, None), "NULL")
    assert hip.plane(0, 2).size == 0
    # still a plain handle of its own size
    dev_own = _device_frames(frames[:2], c.dw, c.dh, c.pitch, pad=0)
    hip.track_device_async(dev_own[0, 0].data_ptr(), dev_own[0, 1].data_ptr(), c.dh, c.dw, c.pitch)
    refused(hip, hip.set_rectifiers(r, r), "in flight")                                                           # a frame in flight
    R, t, st = hip.wait_status()
    assert st == 2
    _close_to(R, t, ref[0], "the frame in flight during the refusals")
    hip.close()

    hip = hip_lib.LvtSystem.create(c.prm, 1)
    assert hip.set_rectifiers(r, r) == 0, hip.last_error()
    dev = _device_frames(c.raw[:3], c.sw, c.sh, c.sw)
    own = np.zeros((c.dh, c.dw), np.uint8)
    hip.track_device_async(dev[0, 0].data_ptr(), dev[0, 1].data_ptr(), c.sh, c.sw, c.sw)       # frame 0 in flight through all of the following
    assert hip.last_error() == ""
    assert hip.track_async(own, own) == -1 and "size" in hip.last_error()                       # lvt_amd_track_async: the tracker's own size
    hip.track_device_async(dev_own[0, 0].data_ptr(), dev_own[0, 1].data_ptr(), c.dh, c.dw, c.pitch)
    assert "size" in hip.last_error()                                                           # lvt_amd_track_device_async
    refused(hip, hip.set_rectifiers(None, None), "in flight")                                   # (and no detach under a frame in flight)
    R, t, st = hip.wait_status()
    assert st == 2
    _close_to(R, t, ref[0], "frame 0")
    before = (hip.counts(), hip.get_state())
    assert before[0]["frame"] == ref[0][3]["frame"]
    hip.track(own, own)                                                                         # lvt_track
    assert "size" in hip.last_error()
    hip.track_device(dev_own[0, 0].data_ptr(), dev_own[0, 1].data_ptr(), c.dh, c.dw, c.pitch)  # lvt_amd_track_device
    assert "size" in hip.last_error()
    assert (hip.counts(), hip.get_state()) == before
    R, t = hip.track(*c.raw[1])                                                                 # the handle goes on with the next raw frame
    _close_to(R, t, ref[1], "the frame after the refusals")
    _counts_equal(hip.counts(), ref[1][3], "the frame after the refusals")
    # detached: its own size again, and the source's size is refused
    assert hip.set_rectifiers(None, None) == 0, hip.last_error()
    hip.track(*c.raw[2])
    assert "size" in hip.last_error()
    hip.track(*frames[2])
    _counts_equal(hip.counts(), ref[2][3], "the first frame after the detach")

    # a uniform batch: its one size has to be every sequence's
    batch = hip_lib.LvtBatch(c.prm, 2)
    assert batch.set_rectifiers(1, r, r) == 0, batch.last_error()
    batch.track_device_async([dev_own[0, 0].data_ptr(), dev[0, 0].data_ptr()], [dev_own[0, 1].data_ptr(), dev[0, 1].data_ptr()], c.dh, c.dw, c.pitch)
    assert "size" in batch.last_error()
    refused(batch, batch.set_rectifiers(0, r, r_small), "828 x 250", "500 x 150")
    assert batch.set_rectifiers(0, r, r) == 0, batch.last_error()
    batch.track_device_async([dev[0, 0].data_ptr(), dev[1, 0].data_ptr()], [dev[0, 1].data_ptr(), dev[1, 1].data_ptr()], c.sh, c.sw, c.sw)
    R, t, st = batch.wait()
    assert list(st) == [2, 2]
    _close_to(R[0], t[0], ref[0], "batch sequence 0")


# ---- 6. ownership ---------------------------------------------------------------------------------------------------------------------------------
def test_get_info_round_trips_the_record(hip_lib):
    (sw, sh), (dw, dh), K, R, P = SHAPES["90x50_to_67x35"]
    for model, D in ((RADTAN, RADTAN12), (FISHEYE, [0.6, 0.05, -0.01, 0.002])):
        lens, size = hip_lib.Rectifier.from_lens(hip_lib.Lens(model, sw, sh, K, D), R, P, dw, dh).info()
        assert (lens.model, lens.width, lens.height, size) == (model, sw, sh, (dw, dh))
        assert np.array_equal(lens.K.reshape(-1), np.array(K)) and np.array_equal(lens.D, np.array(list(D) + [0.0] * (12 - len(D))))
    old, size = hip_lib.Rectifier(K, PINCUSHION, EYE3, P, 67, 35).info()
    assert (old.model, old.width, old.height, size) == (RADTAN, 67, 35, (67, 35)) and list(old.D) == PINCUSHION + [0.0] * 7
    L = hip_lib.load_library()
    assert L.lvt_amd_rectifier_get_info(None, None, None) == -1


def test_destroying_a_detached_rectifier_leaves_a_plain_handle(hip_lib, oracle_lib):
    c = get_case("fisheye_strong")
    frames = _library_rect(hip_lib, c)
    hip = hip_lib.LvtSystem.create(c.prm, 1)
    r = c.rectifier(hip_lib)
    assert hip.set_rectifiers(r, r) == 0, hip.last_error()
    hip.track(*c.raw[0])
    assert hip.set_rectifiers(None, None) == 0, hip.last_error()
    r.close()
    orc = oracle_lib.Oracle(c.prm, 1)
    orc.track(*frames[0])
    for i in (1, 2, 3):
        orc.track(*frames[i])
        hip.track(*frames[i])
        assert hip.last_error() == "", hip.last_error()
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
    assert hip.plane(0, 2).size == 0
