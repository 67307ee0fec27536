#!/usr/bin/env python3
"""Sensor formats (lvt_amd_set_sensor_format; k_sensor_frames, k_sensor_hist, k_sensor_levels) measured on one MI355X; writes profiles/sensor_formats.md.

  (a) each launch between its HIP events (the profile slots of a handle that tracks): a KITTI-shaped pair (1240 x 376), a 640 x 480 image (RGB-D) and a batch
      of 16 pairs of 1240 x 376, per format;
  (b) per format, synchronous p50 and frames per second with three in flight, against the parent's routes: `host`, the caller converts on one host core with
      a compiled restatement (g++ -O2) and uses the gray entry points; `torch`, the caller builds the gray plane on the device with torch (integer
      arithmetic, the same bytes) and uses the device entry points; `new`, the sensor's plane goes in as it is;
  (c) handles that never set the property, this commit's library against the parent's (--parent-lib, child processes of their own that alternate): the
      asynchronous stereo route, synchronous lvt_track p50, the synchronous RGB-D route.

Medians of --repeats runs.

  python tools/sensor_formats.py [--parent-lib /path/to/parent/liblvt_c.so] [--out profiles/sensor_formats.md] [--repeats 3]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FRAMES, WARM, DEPTH = 60, 10, 3

HOST_SRC = r"""
#include <cstddef>
#include <cstdint>
static inline int mir(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }
extern "C" void bayer_u8(const uint8_t *s, int w, int h, int rx, int ry, uint8_t *d) {
    for (int y = 0; y < h; y++) {
        const uint8_t *r0 = s + (size_t)mir(y - 1, h) * w, *r1 = s + (size_t)y * w, *r2 = s + (size_t)mir(y + 1, h) * w;
        const bool red_row = (y & 1) == ry;
        for (int x = 0; x < w; x++) {
            const int xl = mir(x - 1, w), xr = mir(x + 1, w);
            const unsigned C4 = 4u * r1[x], Hs = r1[xl] + r1[xr], Vs = r0[x] + r2[x], Ds = r0[xl] + r0[xr] + r2[xl] + r2[xr];
            const bool red_col = (x & 1) == rx;
            unsigned R4, G4, B4;
            if (red_row == red_col) G4 = Hs + Vs, R4 = red_row ? C4 : Ds, B4 = red_row ? Ds : C4;
            else G4 = C4, R4 = red_row ? 2 * Hs : 2 * Vs, B4 = red_row ? 2 * Vs : 2 * Hs;
            d[(size_t)y * w + x] = (uint8_t)((4899u * R4 + 9617u * G4 + 1868u * B4 + 32768u) >> 16);
        }
    }
}
extern "C" void luma_u8(const uint8_t *s, int w, int h, int first, uint8_t *d) {
    for (size_t i = 0, n = (size_t)w * h; i < n; i++) d[i] = s[2 * i + first];
}
extern "C" void mono16_u8(const uint16_t *s, int w, int h, int aut, int lo, int hi, int lo_pm, int hi_pm, int span, uint8_t *d) {
    const size_t n = (size_t)w * h;
    if (aut) {
        static unsigned hist[4096];
        for (int b = 0; b < 4096; b++) hist[b] = 0;
        for (size_t i = 0; i < n; i++) hist[s[i] >> 4]++;
        unsigned long long cum = 0;
        int lb = -1, hb = -1;
        for (int b = 0; b < 4096 && hb < 0; b++) {
            cum += hist[b];
            if (lb < 0 && cum * 1000ull > (unsigned long long)lo_pm * n) lb = b;
            if (cum * 1000ull >= (unsigned long long)(1000 - hi_pm) * n) hb = b;
        }
        lo = 16 * lb, hi = 16 * hb + 15;
        if (hi - lo < span) {
            const int mid = (lo + hi) >> 1;
            lo = mid - (span >> 1) < 0 ? 0 : mid - (span >> 1), hi = lo + span;
            if (hi > 65535) hi = 65535, lo = hi - span;
        }
    }
    const unsigned dd = hi - lo;
    for (size_t i = 0; i < n; i++) {
        const unsigned g = s[i] < lo ? lo : (s[i] > hi ? hi : s[i]);
        d[i] = (uint8_t)(((g - lo) * 255u + (dd >> 1)) / dd);
    }
}
"""


def host_converter():
    import sensor_util as SU
    d = tempfile.mkdtemp()
    src, lib = os.path.join(d, "s.cpp"), os.path.join(d, "s.so")
    open(src, "w").write(HOST_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    vp, i = C.c_void_p, C.c_int
    L.bayer_u8.argtypes = [vp, i, i, i, i, vp]
    L.luma_u8.argtypes = [vp, i, i, i, vp]
    L.mono16_u8.argtypes = [vp, i, i, i, i, i, i, i, i, vp]

    def convert(a, rec):
        if rec.format in SU.BAYER:
            out = np.empty(a.shape, np.uint8)
            L.bayer_u8(a.ctypes.data, a.shape[1], a.shape[0], *SU.RED[rec.format], out.ctypes.data)
        elif rec.format in (SU.YUYV, SU.UYVY):
            out = np.empty((a.shape[0], a.shape[1] // 2), np.uint8)
            L.luma_u8(a.ctypes.data, out.shape[1], out.shape[0], 0 if rec.format == SU.YUYV else 1, out.ctypes.data)
        else:
            out = np.empty(a.shape, np.uint8)
            L.mono16_u8(a.ctypes.data, a.shape[1], a.shape[0], rec.auto_window, rec.lo, rec.hi, rec.lo_permille, rec.hi_permille, rec.min_span, out.ctypes.data)
        return out
    return convert


def torch_convert(t, rec, SU):
    """the gray plane on the device with torch, integer arithmetic: the same bytes as the definition"""
    import torch
    import torch.nn.functional as F
    if rec.format in (SU.YUYV, SU.UYVY):
        return t[:, (0 if rec.format == SU.YUYV else 1)::2].contiguous()
    if rec.format == SU.MONO16:
        v = t.to(torch.int32)
        if rec.auto_window:
            hist = torch.bincount((v >> 4).reshape(-1), minlength=4096)
            cum = torch.cumsum(hist, 0)
            N = v.numel()
            lb = int(torch.nonzero(cum * 1000 > rec.lo_permille * N)[0])
            hb = int(torch.nonzero(cum * 1000 >= (1000 - rec.hi_permille) * N)[0])
            lo, hi = 16 * lb, 16 * hb + 15
            if hi - lo < rec.min_span:
                mid = (lo + hi) >> 1
                lo = max(0, mid - (rec.min_span >> 1)); hi = lo + rec.min_span
                if hi > 65535:
                    hi = 65535; lo = hi - rec.min_span
        else:
            lo, hi = rec.lo, rec.hi
        g = v.clamp(lo, hi)
        return torch.div((g - lo) * 255 + ((hi - lo) >> 1), hi - lo, rounding_mode="floor").to(torch.uint8)
    p = F.pad(t.to(torch.int32)[None, None], (1, 1, 1, 1), mode="reflect")[0, 0]
    c, hs, vs = p[1:-1, 1:-1], p[1:-1, :-2] + p[1:-1, 2:], p[:-2, 1:-1] + p[2:, 1:-1]
    ds = p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:]
    rx, ry = SU.RED[rec.format]
    H, W = t.shape
    yy = (torch.arange(H, device=t.device)[:, None] & 1) == ry
    xx = (torch.arange(W, device=t.device)[None, :] & 1) == rx
    at_r, at_b = yy & xx, ~yy & ~xx
    R4 = torch.where(at_r, 4 * c, torch.where(at_b, ds, torch.where(yy, 2 * hs, 2 * vs)))
    B4 = torch.where(at_b, 4 * c, torch.where(at_r, ds, torch.where(yy, 2 * vs, 2 * hs)))
    G4 = torch.where(at_r | at_b, hs + vs, 4 * c)
    return ((4899 * R4 + 9617 * G4 + 1868 * B4 + 32768) >> 16).to(torch.uint8)


def world_of(kind, size, n=4):
    import lvt_amd
    from lvt_amd.synth import make_world
    w = make_world(kind, seed=3, size=size)
    kw = dict(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy)
    if kind == "kitti":
        kw["baseline"] = w.baseline
        return w, lvt_amd.kitti_params(**kw), [tuple(np.ascontiguousarray(x) for x in w.render_stereo(i)) for i in range(n)]
    return w, lvt_amd.tum_params(**kw), [tuple(np.ascontiguousarray(x) for x in w.render_rgbd(i)) for i in range(n)]


def records():
    import sensor_util as SU
    return [("RGGB8", SU.Record(SU.RGGB)), ("YUYV", SU.Record(SU.YUYV)), ("MONO16 fixed", SU.Record(SU.MONO16, lo=19990, hi=20790)), ("MONO16 auto", SU.THERMAL)]


def sensor_plane_of(gray, rec, seed):
    import colour_util as CU
    import sensor_util as SU
    if rec.format in SU.BAYER:
        return SU.mosaic(*CU.colour_channels(gray, 3, seed, 0)[:3], rec.format)
    if rec.format in (SU.YUYV, SU.UYVY):
        return SU.yuv422_of_gray(gray, rec.format, seed)
    return SU.thermal(gray, seed)


def timed_sync(track, n=FRAMES, warm=WARM):
    ts = []
    for i in range(n + warm):
        t0 = time.perf_counter()
        track(i)
        if i >= warm:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e6


def timed_flight(submit, wait, n=4 * FRAMES, warm=WARM):
    inflight = 0
    for i in range(warm):
        submit(i)
        wait()
    t0 = time.perf_counter()
    for i in range(n):
        submit(i)
        inflight += 1
        if inflight >= DEPTH:
            wait(); inflight -= 1
    while inflight:
        wait(); inflight -= 1
    return n / (time.perf_counter() - t0)


def leg_launches(out):
    """(a): the profile slots"""
    import lvt_amd
    _, prm, frames = world_of("kitti", (1240, 376))
    _, prm2, rg = world_of("tum", (640, 480))
    for name, rec in records():
        cfg = lvt_amd.SensorFormat(**rec.fields())
        row = {}
        for what, sensor, p, make in (("pair 1240 x 376", 1, prm, None), ("image 640 x 480", 2, prm2, None)):
            hip = lvt_amd.LvtSystem.create(p, sensor)
            assert hip.set_sensor_format(cfg) == 0, hip.last_error()
            if sensor == 1:
                planes = [tuple(sensor_plane_of(g, rec, 2 * i + e) for e, g in enumerate(frames[i])) for i in range(4)]
                run = lambda i: hip.track(*planes[i % 4])
            else:
                planes = [sensor_plane_of(rg[i][0], rec, i) for i in range(4)]
                run = lambda i: hip.track(planes[i % 4], rg[i % 4][1].astype(np.float32))
            for i in range(WARM):
                run(i)
            hip.profile_enable(True)
            for i in range(FRAMES):
                run(i)
            row[what] = {n: ms / calls * 1e3 for n, ms, calls in hip.profile_read() if n.startswith("k_sensor") and calls}
            hip.close()
        B = 16
        batch = lvt_amd.LvtBatch(prm, B)
        for s in range(B):
            assert batch.set_sensor_format(s, cfg) == 0, batch.last_error()
        import torch
        planes = [tuple(sensor_plane_of(g, rec, 2 * i + e) for e, g in enumerate(frames[i])) for i in range(4)]
        dev = [[torch.from_numpy(p.view(np.uint8).reshape(p.shape[0], -1).copy()).cuda() for p in pair] for pair in planes]
        pitch = dev[0][0].shape[1]
        batch.profile_enable(False)
        for i in range(WARM + FRAMES):
            if i == WARM:
                batch.profile_enable(True)
            batch.track_device_async([dev[i % 4][0].data_ptr()] * B, [dev[i % 4][1].data_ptr()] * B, 376, 1240, pitch)
            batch.wait()
        row["batch of 16 pairs"] = {n: ms / calls * 1e3 for n, ms, calls in batch.profile_read() if n.startswith("k_sensor") and calls}
        out[name] = row


def leg_routes(out):
    """(b): per format, the three routes on the stereo world"""
    import torch
    import lvt_amd
    import sensor_util as SU
    _, prm, frames = world_of("kitti", (1240, 376))
    conv = host_converter()
    W, H = 1240, 376
    pitch = (W + 63) // 64 * 64
    for name, rec in records():
        planes = [tuple(sensor_plane_of(g, rec, 2 * i + e) for e, g in enumerate(frames[i])) for i in range(4)]
        for pair in planes:   # the compiled restatement and torch agree with numpy before anything is timed
            for p in pair:
                want = SU.convert(p, rec)[0]
                assert np.array_equal(conv(p, rec), want)
                assert np.array_equal(torch_convert(torch.from_numpy(p.view(np.uint8 if p.dtype == np.uint8 else np.int16)).cuda() if p.dtype == np.uint8
                                                    else torch.from_numpy(p.astype(np.int32)).cuda(), rec, SU).cpu().numpy(), want)
        res = {}
        # new
        hip = lvt_amd.LvtSystem.create(prm, 1)
        assert hip.set_sensor_format(lvt_amd.SensorFormat(**rec.fields())) == 0
        res["new sync p50 us"] = timed_sync(lambda i: hip.track(*planes[i % 4]))
        res["new fps"] = timed_flight(lambda i: hip.track_async(*planes[i % 4]), hip.wait)
        hip.close()
        # host
        hip = lvt_amd.LvtSystem.create(prm, 1)
        res["host sync p50 us"] = timed_sync(lambda i: hip.track(conv(planes[i % 4][0], rec), conv(planes[i % 4][1], rec)))
        keep = []

        def submit_host(i):
            keep.append((conv(planes[i % 4][0], rec), conv(planes[i % 4][1], rec)))
            del keep[:-8]
            hip.track_async(*keep[-1])
        res["host fps"] = timed_flight(submit_host, hip.wait)
        t0 = time.perf_counter()
        for i in range(20):
            conv(planes[i % 4][0], rec)
        res["host convert us per image"] = (time.perf_counter() - t0) / 20 * 1e6
        hip.close()
        # torch
        hip = lvt_amd.LvtSystem.create(prm, 1)
        dev = [[(torch.from_numpy(p).cuda() if p.dtype == np.uint8 else torch.from_numpy(p.astype(np.int32)).cuda()) for p in pair] for pair in planes]
        ring = [torch.zeros((2, H, pitch), dtype=torch.uint8, device="cuda") for _ in range(8)]

        def submit_torch(i, sync=False):
            buf = ring[i % 8]
            for e in (0, 1):
                buf[e, :, :W] = torch_convert(dev[i % 4][e], rec, SU)
            torch.cuda.synchronize()
            if sync:
                hip.track_device(buf[0].data_ptr(), buf[1].data_ptr(), H, W, pitch)
            else:
                hip.track_device_async(buf[0].data_ptr(), buf[1].data_ptr(), H, W, pitch)
        res["torch sync p50 us"] = timed_sync(lambda i: submit_torch(i, True))
        res["torch fps"] = timed_flight(submit_torch, hip.wait)
        hip.close()
        out[name] = res


def leg_plain(out):
    """(c): handles that never set the property (run once per library, in a child process)"""
    import lvt_amd
    _, prm, frames = world_of("kitti", (1240, 376))
    hip = lvt_amd.LvtSystem.create(prm, 1)
    out["stereo async fps"] = timed_flight(lambda i: hip.track_async(*frames[i % 4]), hip.wait)
    out["lvt_track p50 us"] = timed_sync(lambda i: hip.track(*frames[i % 4]))
    hip.close()
    _, prm2, rg = world_of("tum", (640, 480))
    hip = lvt_amd.LvtSystem.create(prm2, 2)
    depth = [np.ascontiguousarray(f[1], dtype=np.float32) for f in rg]
    out["rgbd sync p50 us"] = timed_sync(lambda i: hip.track(rg[i % 4][0], depth[i % 4]))
    hip.close()


def child(leg, lib=None):
    env = dict(os.environ)
    if lib:
        env["LVT_AMD_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
    print(f"leg {leg}{' (parent)' if lib else ''}: done", file=sys.stderr, flush=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def med(runs, *keys):
    vals = []
    for r in runs:
        for k in keys:
            r = r[k]
        vals.append(r)
    return statistics.median(vals), min(vals), max(vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensor_formats.md"))
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.leg:
        out = {}
        {"launches": leg_launches, "routes": leg_routes, "plain": leg_plain}[a.leg](out)
        print(json.dumps(out))
        return
    launches = [child("launches") for _ in range(a.repeats)]
    routes = [child("routes") for _ in range(a.repeats)]
    plain_new, plain_old = [], []
    for _ in range(a.repeats):   # alternated
        plain_new.append(child("plain"))
        if a.parent_lib:
            plain_old.append(child("plain", a.parent_lib))
    L = ["# Sensor formats: what the conversion costs", "",
         f"One MI355X; medians of {a.repeats} runs (min ... max); `tools/sensor_formats.py` wrote this file.", "",
         "## (a) each launch between its HIP events, microseconds", "", "| format | shape | k_sensor_frames | k_sensor_hist | k_sensor_levels |", "|---|---|---|---|---|"]
    for name in launches[0]:
        for shape in launches[0][name]:
            cells = []
            for k in ("k_sensor_frames", "k_sensor_hist", "k_sensor_levels"):
                cells.append("%.1f (%.1f ... %.1f)" % med(launches, name, shape, k) if k in launches[0][name][shape] else "-")
            L.append(f"| {name} | {shape} | " + " | ".join(cells) + " |")
    L += ["", "## (b) a 1240 x 376 stereo pair per format: the sensor's plane handed in (`new`) against the parent's routes", "",
          "`host`: one host core converts with a compiled restatement (g++ -O2), gray entry points.  `torch`: torch converts on the device (integer arithmetic, the same",
          "bytes), device entry points.  Synchronous p50 in microseconds; frames per second with three in flight.", "",
          "| format | new p50 | host p50 | torch p50 | new fps | host fps | torch fps | host convert, us per image |", "|---|---|---|---|---|---|---|---|"]
    for name in routes[0]:
        c = ["%.0f" % med(routes, name, k)[0] for k in ("new sync p50 us", "host sync p50 us", "torch sync p50 us", "new fps", "host fps", "torch fps", "host convert us per image")]
        L.append(f"| {name} | " + " | ".join(c) + " |")
    L += ["", "## (c) handles that never set the property", "", "| route | this commit | parent |", "|---|---|---|"]
    for k in plain_new[0]:
        new = "%.1f (%.1f ... %.1f)" % med(plain_new, k)
        old = "%.1f (%.1f ... %.1f)" % med(plain_old, k) if plain_old else "not run"
        L.append(f"| {k} | {new} | {old} |")
    L.append("")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    main()
