"""The rectifier's kernels -- k_rectify_map, k_rectify, k_rectify_fix, k_rectify_frames -- at the places where their arithmetic branches.  No expected value
comes from this library: planes are compared byte for byte, maps bit for bit (or NaN for NaN), with the numpy restatement of "RECTIFICATION"
(remap_util, which tests/test_remap_cases.py holds to hand-computed answers and to the oracle), on the planted inputs of remap_cases.  The largest image
is 65 x 33, apart from two sources of 32770 x 1 and 1 x 32770 that the +-32768 clamp needs in order to show."""
import ctypes as C

import numpy as np
import pytest

import remap_cases as RC
import remap_util as RU
from parity_util import diff_frame
from test_gpu_colour_frames import device_colour
from test_gpu_raw_frames import close_to

pytestmark = pytest.mark.gpu

GUARD = 256
TRACKER_ANGLE = 10.0    # degrees about y in the tracker-level case: the oracle is TRACKING on all three frames at the angle first chosen


def guarded(n_bytes):
    """a device buffer of 0xAB with GUARD bytes in front of and behind the n_bytes a call may write; (tensor, address of the writable part)"""
    import torch
    t = torch.full((GUARD + n_bytes + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 4 == 0
    return t, t.data_ptr() + GUARD


def split(t, dh, dpitch, what):
    """the plane out of a guarded buffer, after asserting that no byte outside it was written"""
    got = t.cpu().numpy()
    assert (got[:GUARD] == 0xAB).all() and (got[GUARD + dh * dpitch:] == 0xAB).all(), f"{what}: bytes outside the plane were written"
    return got[GUARD:GUARD + dh * dpitch].reshape(dh, dpitch)


def assert_equal_planes(got, want, dw, what):
    bad = np.argwhere(got[:, :dw] != want[:, :dw])
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at {tuple(bad[0])}: hip {got[tuple(bad[0])]} numpy {want[tuple(bad[0])]}"
    assert not got[:, dw:].any(), f"{what}: the padding columns are not zero"


# ---- 1. every planted case through both routes of the stage entry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_planted_case_equals_numpy_through_both_routes(hip_lib, name):
    """lvt_amd_remap_device, route 0 (k_rectify) and route 1 (k_rectify_fix + k_rectify_frames): the source 0 ... 3 bytes past an aligned address with a pitch
    of sw + 5 and 255 in every byte that is no pixel; the destination inside a buffer of 0xAB at the tightest pitch and at a 64-byte multiple.  The plane is
    numpy's byte for byte, its padding columns zero, every byte outside it untouched, and the two routes agree"""
    src, m1, m2 = RC.CASES[name]
    sh, sw = src.shape
    dh, dw = m1.shape
    k = sorted(RC.CASES).index(name)
    for dpitch in ((dw + 3) // 4 * 4, (dw + 63) // 64 * 64 + (64 if dw % 64 == 0 else 0)):
        want, _ = RU.remap(src, m1, m2, out_pitch=dpitch)
        planes = []
        for route in (0, 1):
            keep, d_src, spitch = device_colour(src[:, :, None], k % 4)
            assert spitch == sw + 5 and d_src % 4 == k % 4
            t, d_dst = guarded(dh * dpitch)
            rc, launches = hip_lib.remap_device(d_src, sw, sh, spitch, m1, m2, d_dst, dpitch, route)
            assert (rc, launches) == (0, 1 + route), (name, route, hip_lib.last_call_error())
            got = split(t, dh, dpitch, f"{name} route {route} pitch {dpitch}")
            assert_equal_planes(got, want, dw, f"{name} route {route} pitch {dpitch} offset {k % 4}")
            planes.append(got)
            k += 1
        assert np.array_equal(planes[0], planes[1]), f"{name}: route 0 and route 1 differ"


# ---- 2. every calibration through a Rectifier -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.CALIBRATIONS))
def test_calibration_through_a_rectifier_equals_numpy(hip_lib, name):
    """k_rectify_map's maps are rectify_maps' (bits, or NaN for NaN); rectify() and rectify_device() of a noise image and of an all-255 image are remap's"""
    K, D, R, P, w, h = RC.CALIBRATIONS[name]
    want_maps = RU.rectify_maps(K, D, R, P, w, h)
    rect = hip_lib.Rectifier(K, D, R, P, w, h)
    maps = rect.maps()
    for k in (0, 1):
        bad = np.argwhere(~((np.isnan(maps[k]) & np.isnan(want_maps[k])) | (maps[k].view(np.uint32) == want_maps[k].view(np.uint32))))
        assert len(bad) == 0, f"{name} map{k + 1}: {len(bad)} entries differ, first at {tuple(bad[0])}: hip {maps[k][tuple(bad[0])]!r} numpy {want_maps[k][tuple(bad[0])]!r}"
    dpitch = (w + 3) // 4 * 4
    for j, img in enumerate((np.random.default_rng(w * 100 + h).integers(0, 256, (h, w), dtype=np.uint8), np.full((h, w), 255, np.uint8))):
        want, _ = RU.remap(img, *want_maps, out_pitch=dpitch)
        got = rect.rectify(img)
        assert got.shape == (h, w)
        assert_equal_planes(got, want[:, :w], w, f"{name} rectify image {j}")
        keep, d_src, spitch = device_colour(img[:, :, None], 1 + j)
        t, d_dst = guarded(h * dpitch)
        assert rect.rectify_device(d_src, spitch, d_dst, dpitch) == 0
        import torch
        torch.cuda.synchronize()
        assert_equal_planes(split(t, h, dpitch, f"{name} rectify_device image {j}"), want, w, f"{name} rectify_device image {j}")
    rect.close()


# ---- 3. one tracker-level case ------------------------------------------------------------------------------------------------------------------
def test_a_tracker_with_a_rotated_calibration_equals_the_oracle_on_numpy_frames(hip_lib, oracle_lib):
    """case A's world of test_gpu_raw_frames.py (kitti 71 at 621 x 187) with rotated_10deg's distortion and rotation as the calibration of both eyes, one handle,
    three frames: plane 2 is remap of the raw frame, and the oracle fed the restatement's rectified frames agrees frame by frame"""
    from test_gpu_raw_frames import get_case
    c = get_case("A")
    W, H = c.W, c.H
    K = [c.world.fx, 0.0, c.world.cx, 0.0, c.world.fy, c.world.cy, 0.0, 0.0, 1.0]
    D, R = RC.CALIBRATIONS["rotated_10deg"][1], RC._rot_y(TRACKER_ANGLE)
    assert R == RC.CALIBRATIONS["rotated_10deg"][2]
    maps = RU.rectify_maps(K, D, R, K, W, H)
    rect = [tuple(RU.remap(img, *maps)[0] for img in pair) for pair in c.raw[:3]]
    orc = c.oracle()
    states = []
    for pair in rect:
        orc.track(*pair)
        states.append(orc.status)
    assert states == [2, 2, 2], f"the oracle is not TRACKING on every frame at {TRACKER_ANGLE} degrees: {states}"
    rl = hip_lib.Rectifier(K, D, R, K, W, H)
    assert all(RU.maps_equal(a, b) for a, b in zip(rl.maps(), maps))
    hip, orc = hip_lib.LvtSystem.create(c.prm, 1), c.oracle()
    assert hip.set_rectifiers(rl, rl) == 0, hip.last_error()
    for i in range(3):
        Ro, to = orc.track(*rect[i])
        Rh, th = hip.track(*c.raw[i])
        assert hip.last_error() == "", hip.last_error()
        for eye in (0, 1):
            p = hip.plane(eye, 2)
            assert p.shape == (H, c.pitch)
            assert_equal_planes(p, rect[i][eye], W, f"frame {i} eye {eye}")
        msgs = diff_frame(hip, orc)
        assert not msgs, (i, msgs[:6])
        close_to(Rh, th, (np.array(Ro), np.array(to)), f"frame {i}")


# ---- 4. refusals of the stage entry ---------------------------------------------------------------------------------------------------------------
def test_the_stage_entry_refuses_bad_arguments(hip_lib):
    """each refusal's sentence, a launch count of 0, and a destination no byte of which was written"""
    import torch
    L = hip_lib.load_library()
    src = torch.full((64,), 9, dtype=torch.uint8, device="cuda")
    m = np.full((4, 4), 1.0, np.float32)
    t, d_dst = guarded(64)
    ok = dict(d_src=src.data_ptr(), sw=4, sh=4, spitch=4, m1=m.ctypes.data, m2=m.ctypes.data, dw=4, dh=4, d_dst=d_dst, dpitch=4, route=0)

    def call(**change):
        a = dict(ok, **change)
        n = C.c_int(7)
        rc = L.lvt_amd_remap_device(C.c_void_p(a["d_src"]), a["sw"], a["sh"], a["spitch"], C.c_void_p(a["m1"]), C.c_void_p(a["m2"]), a["dw"], a["dh"],
                                    C.c_void_p(a["d_dst"]), a["dpitch"], a["route"], C.byref(n))
        return rc, n.value, hip_lib.last_call_error()
    who = "lvt_amd_remap_device: "
    null = who + "a NULL argument (nothing was launched)"
    size = who + "a size that is not positive (nothing was launched)"
    spitch = who + "a source pitch smaller than the source width (nothing was launched)"
    dpitch = who + "a destination pitch smaller than the map width or no multiple of 4, or a destination that is not 4-byte aligned (nothing was launched)"
    big = who + "a plane of more than INT_MAX bytes (nothing was launched)"
    refused = [(dict(d_src=None), null), (dict(m1=None), null), (dict(m2=None), null), (dict(d_dst=None), null),
               (dict(sw=0), size), (dict(sh=0), size), (dict(dw=0), size), (dict(dh=0), size), (dict(sw=-4), size), (dict(dh=-1), size),
               (dict(spitch=3), spitch), (dict(dpitch=0), dpitch), (dict(dw=3, dpitch=2), dpitch), (dict(dw=3, dpitch=3), dpitch), (dict(dpitch=6), dpitch),
               (dict(d_dst=d_dst + 2), dpitch),
               (dict(spitch=1 << 20, sh=1 << 12), big), (dict(dpitch=1 << 20, dh=1 << 12), big), (dict(sw=1 << 16, spitch=1 << 16, sh=1 << 15), big),
               (dict(route=2), who + "unknown route 2 (nothing was launched)"), (dict(route=-1), who + "unknown route -1 (nothing was launched)")]
    for change, sentence in refused:
        assert call(**change) == (-1, 0, sentence), change
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == 0xAB).all(), "a refused call wrote to the destination"
    # (and the same arguments unchanged are taken: a 4 x 4 source of 9 under an all-integer map is 9 everywhere)
    assert call()[:2] == (0, 1) and call(route=1)[:2] == (0, 2)
    assert (split(t, 4, 4, "accepted call") == 9).all()
