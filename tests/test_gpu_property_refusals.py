"""The refusals of the calls that change a property of a handle -- lvt_amd_set_rectifiers, lvt_amd_set_pixel_format, lvt_amd_set_depth_camera,
lvt_amd_enable_pose_info, lvt_amd_snapshot_apply and their batch spellings -- on a solo handle, a uniform batch of 2, a pooled seat, an automatic seat and a
handle of the other sensor.  Every refusal returns -1 and leaves the COMPLETE sentence below in lvt_amd_last_error (callers match on these texts); where two
objections apply at once the one named here is the one reported; and after every refusal the handle tracks its next frame to TRACKING.
(Accepted calls, and what counts as a use of an lvt_create handle, are held by the tests of each property.)"""
import ctypes as C

import numpy as np
import pytest

import depth_reg_util as D
from parity_util import make_case

pytestmark = pytest.mark.gpu

U = " (nothing was changed)"
RECT, PIX, DCAM, PINFO = "lvt_amd_set_rectifiers: ", "lvt_amd_set_pixel_format: ", "lvt_amd_set_depth_camera: ", "lvt_amd_enable_pose_info: "
APPLY, BAPPLY = "lvt_amd_snapshot_apply: ", "lvt_amd_batch_snapshot_apply: "
RIDES = "a pooled handle (its frames ride a chain shared with other handles)" + U
TEXT = {
    # the handle's kind
    "rect pooled": RECT + RIDES,
    "pix pooled": PIX + RIDES,
    "dcam pooled": DCAM + "a pooled handle (pooled handles are stereo only)" + U,
    "pinfo pooled": PINFO + RIDES,
    "apply pooled": APPLY + "a pooled or automatic seat (its state lives in a chain shared with other handles)" + U,
    "rect rgbd": RECT + "an RGB-D handle (there is one image, and its depth plane is registered to it)" + U,
    "dcam stereo": DCAM + "a stereo handle (it has no depth plane to register)" + U,
    # the spelling
    "rect solo call on a batch": RECT + "a batch handle takes its rectifiers per sequence through lvt_amd_batch_set_rectifiers" + U,
    "pix solo call on a batch": PIX + "a batch handle takes its pixel formats per sequence through lvt_amd_batch_set_pixel_format" + U,
    "dcam solo call on a batch": DCAM + "a batch handle takes its depth cameras per sequence through lvt_amd_batch_set_depth_camera" + U,
    "pix batch call on a solo": PIX + "lvt_amd_batch_set_pixel_format on a handle that is not a batch (use lvt_amd_set_pixel_format)" + U,
    "dcam batch call on a solo": DCAM + "lvt_amd_batch_set_depth_camera on a handle that is not a batch (use lvt_amd_set_depth_camera)" + U,
    "bapply on a solo": BAPPLY + "a batch call on a handle that is not a batch" + U,
    # the sequence
    "rect seq 1 of a solo": RECT + "no sequence 1 in this handle" + U,
    "rect seq 2": RECT + "no sequence 2 in this handle" + U,
    "rect seq -1": RECT + "no sequence -1 in this handle" + U,
    "pix seq 2": PIX + "no sequence 2 in this handle" + U,
    "dcam seq 2": DCAM + "no sequence 2 in this handle" + U,
    "apply seq 2 of a solo": APPLY + "no sequence 2 in this handle (seq is 0 for a solo handle)" + U,
    "apply seq 2": APPLY + "no sequence 2 in this handle" + U,
    # the value
    "rect one NULL": RECT + "one rectifier is NULL (both, or NULL, NULL to detach)" + U,
    "rect size": RECT + "a rectifier of 613 x 185 on a sequence of 620 x 188" + U,
    "pix unknown": PIX + "unknown pixel format 99" + U,
    "dcam size": DCAM + "a depth camera of 0 x 240 pixels (1 ... 8192 each way)" + U,
    "dcam size 8193": DCAM + "a depth camera of 320 x 8193 pixels (1 ... 8192 each way)" + U,
    "dcam non-finite": DCAM + "a depth camera with a non-finite field" + U,
    "dcam focal": DCAM + "a depth camera whose fx or fy is not > 0" + U,
    "apply not a snapshot": APPLY + "not a snapshot" + U,
    "apply parameters": APPLY + "the snapshot's parameters differ from the sequence's" + U,
    "apply sensor": APPLY + "a snapshot of sensor type 2 on a handle of sensor type 1" + U,
    "apply parameters, sequence 1": APPLY + "sequence 1: the snapshot's parameters differ from the sequence's" + U,
    "bapply parameters, sequence 1": BAPPLY + "sequence 1: the snapshot's parameters differ from the sequence's" + U,
    # a quiet handle
    "rect in flight": RECT + "frames in flight: attach before the first frame or after every frame has been collected" + U,
    "pix in flight": PIX + "frames in flight: set the format before the first frame or after every frame has been collected" + U,
    "dcam in flight": DCAM + "frames in flight: set the camera before the first frame or after every frame has been collected" + U,
    "pinfo in flight": PINFO + "frames in flight: enable before the first frame or after every frame has been collected" + U,
    "apply in flight": APPLY + "frames in flight: apply after every frame has been collected" + U,
}
RGB8 = 2


def pingpong(i, n):
    i %= 2 * n - 2
    return i if i < n else 2 * n - 2 - i


class Stereo:
    """the half-size KITTI world's frames, on the host and in HBM"""

    def __init__(self, n=28):
        import torch
        self.world, self.prm, _ = make_case("kitti", 0, 0.5)
        self.W, self.H, self.n = self.world.W, self.world.H, n
        assert (self.W, self.H) == (620, 188)
        self.pitch = ((self.W + 63) // 64) * 64
        self.frames = [tuple(np.ascontiguousarray(x) for x in self.world.render_stereo(i)) for i in range(n)]
        self.dev = torch.zeros((n, 2, self.H, self.pitch), dtype=torch.uint8, device="cuda")
        for i, (a, b) in enumerate(self.frames):
            self.dev[i, 0, :, :self.W] = torch.from_numpy(a).cuda(); self.dev[i, 1, :, :self.W] = torch.from_numpy(b).cuda()
        torch.cuda.synchronize()


class Checked:
    """a handle, how it takes its next frame, and the check every refusal gets"""

    def __init__(self, h, track):
        self.h, self._track, self.i, self.seen = h, track, 0, []

    def next_frame(self):
        st = self._track(self.i)
        self.i += 1
        assert list(np.atleast_1d(st)) == [2] * len(np.atleast_1d(st)), (self.i, st, self.h.last_error())

    def refused(self, rc, key):
        assert rc == -1 and self.h.last_error() == TEXT[key], (key, rc, self.h.last_error())
        self.seen.append(key)
        self.next_frame()


def rectifier(hip_lib, w, h):
    K = [300.0, 0.0, w / 2.0, 0.0, 300.0, h / 2.0, 0.0, 0.0, 1.0]
    return hip_lib.Rectifier(K, [0.05, 0.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], K, w, h)


def edited(cam, **kw):
    c = D.make_camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, cam.R, cam.t)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_every_refusal_says_its_sentence_and_changes_nothing(hip_lib, tmp_path):
    L = hip_lib.load_library()
    vp = C.c_void_p
    S = Stereo()
    rl, other = rectifier(hip_lib, S.W, S.H), rectifier(hip_lib, 613, 185)
    q = D.sequence("plain")          # 320 x 240 RGB-D, registered depth
    cam = D.sequence("same").cam
    from test_gpu_depth_registration import planes
    P = planes("plain")
    seen = []

    def stereo_track(h):
        def go(i):
            h.track(*S.frames[pingpong(i, S.n)])
            return h.get_state()
        return go

    # ---- a solo stereo handle ------------------------------------------------------------------------------------------------------------------
    hip = hip_lib.LvtSystem.create(S.prm, 1)
    k = Checked(hip, stereo_track(hip))
    k.next_frame(); k.next_frame()
    good = hip.snapshot()
    _, other_prm, _ = make_case("kitti", 0, 0.5, {"tracking_radius": 30})
    X = hip_lib.LvtSystem.create(other_prm, 1)
    sx = X.snapshot()
    X.close()
    R = hip_lib.LvtSystem.create(q.prm, 2)
    sd = R.snapshot()
    R.close()
    k.refused(hip.set_rectifiers(other, other), "rect size")
    k.refused(hip.set_rectifiers(rl, None), "rect one NULL")
    k.refused(hip.set_rectifiers(None, rl), "rect one NULL")
    k.refused(L.lvt_amd_batch_set_rectifiers(vp(hip._h), 1, vp(rl._h), vp(rl._h)), "rect seq 1 of a solo")   # (the batch spelling is accepted for seq 0: below)
    k.refused(hip.set_pixel_format(99), "pix unknown")
    k.refused(L.lvt_amd_batch_set_pixel_format(vp(hip._h), 0, RGB8), "pix batch call on a solo")
    k.refused(L.lvt_amd_batch_set_pixel_format(vp(hip._h), 5, RGB8), "pix batch call on a solo")             # precedence: the spelling before the sequence
    k.refused(hip.set_depth_camera(cam), "dcam stereo")
    k.refused(L.lvt_amd_batch_set_depth_camera(vp(hip._h), 0, C.byref(cam)), "dcam stereo")
    k.refused(L.lvt_amd_snapshot_apply(vp(hip._h), 2, vp(good._h)), "apply seq 2 of a solo")
    k.refused(L.lvt_amd_batch_snapshot_apply(vp(hip._h), (vp * 1)(good._h)), "bapply on a solo")
    k.refused(hip.restore(None), "apply not a snapshot")
    k.refused(hip.restore(sx), "apply parameters")
    k.refused(hip.restore(sd), "apply sensor")
    # frames in flight: every call, and the value before the quiet handle
    for call, key in ((lambda: hip.set_rectifiers(rl, rl), "rect in flight"), (lambda: hip.set_rectifiers(other, other), "rect size"),
                      (lambda: hip.set_pixel_format(RGB8), "pix in flight"), (lambda: hip.set_pixel_format(99), "pix unknown"),
                      (lambda: hip.enable_pose_info(True), "pinfo in flight"), (lambda: hip.restore(good), "apply in flight"), (lambda: hip.restore(sx), "apply parameters")):
        j = pingpong(k.i, S.n)
        hip.track_device_async(S.dev[j, 0].data_ptr(), S.dev[j, 1].data_ptr(), S.H, S.W, S.pitch)
        rc = call()
        assert rc == -1 and hip.last_error() == TEXT[key], (key, rc, hip.last_error())
        k.seen.append(key)
        assert hip.wait_status()[2] == 2
        k.i += 1
    k.next_frame()
    assert L.lvt_amd_batch_set_rectifiers(vp(hip._h), 0, vp(rl._h), vp(rl._h)) == 0, hip.last_error()        # the deliberate deviation: accepted for seq 0
    assert hip.set_rectifiers(None, None) == 0
    k.next_frame()
    seen += k.seen
    hip.close()

    # ---- a solo RGB-D handle -------------------------------------------------------------------------------------------------------------------
    rg = hip_lib.LvtSystem.create(q.prm, 2)

    def rgbd_track(i):
        rg.track(q.gray[i], q.f32[i])
        return rg.get_state()
    k = Checked(rg, rgbd_track)
    k.next_frame()
    k.refused(rg.set_rectifiers(rl, rl), "rect rgbd")
    k.refused(rg.set_depth_camera(edited(cam, width=0)), "dcam size")
    k.refused(rg.set_depth_camera(edited(cam, height=8193)), "dcam size 8193")
    k.refused(rg.set_depth_camera(edited(cam, cx=float("nan"))), "dcam non-finite")
    k.refused(rg.set_depth_camera(edited(cam, fy=-1.0)), "dcam focal")
    k.refused(L.lvt_amd_batch_set_depth_camera(vp(rg._h), 0, C.byref(cam)), "dcam batch call on a solo")
    k.refused(L.lvt_amd_batch_set_depth_camera(vp(rg._h), 5, C.byref(cam)), "dcam batch call on a solo")       # precedence: the spelling before the sequence
    for call, key in ((lambda: rg.set_depth_camera(cam), "dcam in flight"), (lambda: rg.set_depth_camera(edited(cam, width=0)), "dcam size")):
        ptr, pitch = P.depth(k.i, 0)
        assert rg.track_rgbd_device_async(P.gray(k.i), ptr, q.H, q.W, P.gpitch, pitch, 0, 1.0) == 0, rg.last_error()
        rc = call()
        assert rc == -1 and rg.last_error() == TEXT[key], (key, rc, rg.last_error())
        k.seen.append(key)
        assert rg.wait_status()[2] == 2
        k.i += 1
    k.next_frame()
    assert rg.depth_camera() is None
    seen += k.seen
    rg.close()

    # ---- a uniform stereo batch of 2 -----------------------------------------------------------------------------------------------------------
    b2 = hip_lib.LvtBatch(S.prm, 2)

    def batch_track(i):
        j = pingpong(i, S.n)
        b2.track_device_async([S.dev[j, 0].data_ptr()] * 2, [S.dev[j, 1].data_ptr()] * 2, S.H, S.W, S.pitch)
        return b2.wait()[2]
    k = Checked(b2, batch_track)
    k.next_frame()
    k.refused(L.lvt_amd_set_rectifiers(vp(b2._h), vp(rl._h), vp(rl._h)), "rect solo call on a batch")
    k.refused(L.lvt_amd_set_pixel_format(vp(b2._h), RGB8), "pix solo call on a batch")
    k.refused(b2.set_rectifiers(2, rl, rl), "rect seq 2")
    k.refused(b2.set_rectifiers(-1, rl, rl), "rect seq -1")
    k.refused(b2.set_rectifiers(2, other, other), "rect seq 2")                                                # precedence: the sequence before the value
    k.refused(b2.set_rectifiers(1, other, other), "rect size")
    k.refused(b2.set_pixel_format(2, RGB8), "pix seq 2")
    k.refused(b2.set_pixel_format(2, 99), "pix seq 2")                                                         # precedence: the sequence before the value
    k.refused(b2.set_pixel_format(1, 99), "pix unknown")
    k.refused(b2.set_depth_camera(1, cam), "dcam stereo")
    k.refused(b2.restore(2, good), "apply seq 2")
    k.refused(b2.restore(1, sx), "apply parameters, sequence 1")
    k.refused(b2.restore_all([good, sx]), "bapply parameters, sequence 1")
    seen += k.seen
    b2.close()

    # ---- a uniform RGB-D batch of 2 ------------------------------------------------------------------------------------------------------------
    r2 = hip_lib.LvtBatch(q.prm, 2, 2)

    def rgbd_batch_track(i):
        ptr, pitch = P.depth(i, 0)
        assert r2.track_rgbd_device_async([P.gray(i)] * 2, [ptr] * 2, q.H, q.W, P.gpitch, pitch, 0, 1.0) == 0, r2.last_error()
        return r2.wait()[2]
    k = Checked(r2, rgbd_batch_track)
    k.next_frame()
    k.refused(L.lvt_amd_set_depth_camera(vp(r2._h), C.byref(cam)), "dcam solo call on a batch")
    k.refused(r2.set_depth_camera(2, cam), "dcam seq 2")
    k.refused(r2.set_depth_camera(2, edited(cam, width=0)), "dcam seq 2")                                      # precedence: the sequence before the value
    k.refused(r2.set_depth_camera(1, edited(cam, width=0)), "dcam size")
    k.refused(r2.set_rectifiers(0, rl, rl), "rect rgbd")
    seen += k.seen
    r2.close()

    # ---- a pooled seat and an automatic seat ---------------------------------------------------------------------------------------------------
    S.prm.write_yaml(str(tmp_path / "cfg.yaml"))
    autos = [hip_lib.LvtSystem.create_from_file(str(tmp_path / "cfg.yaml"), 1) for _ in range(2)]
    seat = hip_lib.LvtSystem.create(S.prm, 1, pooled=True)
    assert seat.ordering() == "pooled" and autos[0].ordering() == "pooled"
    for h in (seat, autos[0]):
        k = Checked(h, stereo_track(h))
        k.next_frame()
        k.refused(h.set_rectifiers(rl, rl), "rect pooled")
        k.refused(h.set_pixel_format(RGB8), "pix pooled")
        k.refused(L.lvt_amd_batch_set_pixel_format(vp(h._h), 3, 99), "pix pooled")                             # precedence: the handle's kind before everything
        k.refused(h.set_depth_camera(cam), "dcam pooled")
        k.refused(h.enable_pose_info(True), "pinfo pooled")
        k.refused(h.restore(good), "apply pooled")
        seen += k.seen
    for h in [seat] + autos:
        h.close()
    for s in (good, sx, sd):
        s.close()
    assert set(seen) == set(TEXT), set(TEXT) - set(seen)   # (every sentence of the table was provoked)
