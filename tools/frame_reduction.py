#!/usr/bin/env python3
"""Frame reduction (lvt_amd_set_reduction, k_reduce_frames) measured on one MI355X; writes profiles/frame_reduction.md.

  (a) the launch between its HIP events (the profile slot k_reduce_frames of a handle that tracks): a 2482 x 752 pair at f = 2, a 3840 x 2160 pair at f = 4
      and at f = 8, a batch of 16 pairs of 2482 x 752 at f = 2 -- each on the vector path (planes at an aligned address, pitch % 4 == 0) and on the byte path
      (one byte further, an odd pitch) -- with the bytes per second it moves, beside a device-to-device copy of the same source bytes on the same card;
  (b) the parent's routes against this commit's handle, stereo (1240 x 376 -> 620 x 188) and RGB-D (640 x 480 -> 320 x 240): `host`, the caller reduces on one
      host core with a compiled restatement (g++ -O2) and uses the gray entry points; `torch`, the caller builds the plane on the device with torch (integer
      arithmetic, the same bytes), records an event and uses the device entry points; `new`, the large frame goes in as it is.  Synchronous p50 and frames per
      second with three in flight;
  (c) handles that never set the property against the parent: the asynchronous stereo route, synchronous lvt_track p50, the synchronous RGB-D route;
  (d) a 3840 x 2160 RGB8 pair at f = 4: k_gray_frames and k_reduce_frames, each between its events.

The large frames are the small world's frames with every pixel repeated f x f times: their reduction is the small frame, so the tracker tracks, and nothing is
rendered at 4K.  --parent-lib names the PARENT commit's liblvt_c.so, built from a checkout of its own; its legs run in child processes of their own
(LVT_AMD_LIB) that alternate with this commit's.  Medians of --repeats child runs.

  python tools/frame_reduction.py --parent-lib /path/to/parent/liblvt_c.so [--out profiles/frame_reduction.md] [--resources "..."]
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
FRAMES, WARM, DEPTH = 60, 10, 3

HOST_SRC = r"""
#include <cstddef>
#include <cstdint>
extern "C" void reduce_u8(const uint8_t *s, int sw, int sh, int f, uint8_t *d) {
    const int w = sw / f, h = sh / f;
    const unsigned ff = f * f;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            unsigned S = 0;
            for (int dy = 0; dy < f; dy++)
                for (int dx = 0; dx < f; dx++) S += s[(size_t)(y * f + dy) * sw + x * f + dx];
            d[(size_t)y * w + x] = (uint8_t)((S + ff / 2) / ff);
        }
}
"""


def host_reducer():
    d = tempfile.mkdtemp()
    src, lib = os.path.join(d, "r.cpp"), os.path.join(d, "r.so")
    open(src, "w").write(HOST_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    L.reduce_u8.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]

    def reduce(a, f):
        out = np.empty((a.shape[0] // f, a.shape[1] // f), np.uint8)
        L.reduce_u8(a.ctypes.data, a.shape[1], a.shape[0], f, out.ctypes.data)
        return out
    return reduce


def grow(a, f):
    return np.ascontiguousarray(np.repeat(np.repeat(a, f, axis=0), f, axis=1))


def world_of(kind, size, n=4):
    import lvt_amd
    from lvt_amd.synth import make_world
    w = make_world(kind, seed=3, size=size)
    kw = dict(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy)
    if kind == "kitti":
        kw["baseline"] = w.baseline
        return w, lvt_amd.kitti_params(**kw), [tuple(np.ascontiguousarray(x) for x in w.render_stereo(i)) for i in range(n)]
    return w, lvt_amd.tum_params(**kw), [tuple(np.ascontiguousarray(x) for x in w.render_rgbd(i)) for i in range(n)]


def device_planes(imgs, offset, pitch):
    """images in HBM `offset` bytes past an aligned address, rows `pitch` apart: (owner, [addresses])"""
    import torch
    H, W = imgs[0].shape[:2]
    row = imgs[0].strides[0]
    stride = (H * pitch + 511) // 256 * 256
    buf = np.zeros(len(imgs) * stride + 256, np.uint8)
    for k, a in enumerate(imgs):
        np.lib.stride_tricks.as_strided(buf[k * stride + offset:], shape=(H, row), strides=(pitch, 1))[:] = a.reshape(H, row)
    t = torch.from_numpy(buf).cuda()
    return t, [t.data_ptr() + k * stride + offset for k in range(len(imgs))]


def slot_us(h, name):
    for n, ms, calls in h.profile_read():
        if n == name and calls:
            return 1000.0 * ms / calls
    return None


def copy_us(nbytes):
    import torch
    a = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    for _ in range(5):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(30):
        e0.record(); b.copy_(a); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0)
    return statistics.median(ts)


def child_kernel():
    import lvt_amd
    out = {}
    cases = [("2482 x 752 pair, f = 2", (1241, 376), 2, 1), ("3840 x 2160 pair, f = 4", (960, 540), 4, 1), ("3840 x 2160 pair, f = 8", (480, 270), 8, 1),
             ("16 pairs of 2482 x 752, f = 2", (1241, 376), 2, 16)]
    worlds = {}
    for name, size, f, B in cases:
        if size not in worlds:
            worlds[size] = world_of("kitti", size)
        w, prm, small = worlds[size]
        large = [tuple(grow(a, f) for a in pair) for pair in small]
        fH, fW = large[0][0].shape
        for path, off, pitch in (("vector", 0, (fW + 63) // 64 * 64), ("byte", 1, ((fW + 63) // 64 * 64) | 1)):
            keep, ptr = device_planes([a for pair in large for a in pair], off, pitch)
            if B == 1:
                h = lvt_amd.LvtSystem.create(prm, 1)
                assert h.set_reduction(factor=f, width=fW, height=fH) == 0, h.last_error()
            else:
                h = lvt_amd.LvtBatch(prm, B)
                for s in range(B):
                    assert h.set_reduction(s, factor=f, width=fW, height=fH) == 0, h.last_error()
            for it in range(WARM + FRAMES):
                if it == WARM:
                    h.profile_enable(True)
                k = it % len(large)
                if B == 1:
                    h.track_device_async(ptr[2 * k], ptr[2 * k + 1], fH, fW, pitch)
                    h.wait_status()
                else:
                    h.track_device_async([ptr[2 * k]] * B, [ptr[2 * k + 1]] * B, fH, fW, pitch)
                    h.wait()
            us = slot_us(h, "k_reduce_frames")
            src_bytes = 2 * B * fW * fH
            out[f"{name} | {path}"] = {"us": us, "src_bytes": src_bytes, "dst_bytes": 2 * B * (fW // f) * (fH // f), "copy_us": copy_us(src_bytes), "error": h.last_error()}
            h.close()
    # (d) a 4K RGB8 pair at f = 4
    w, prm, small = worlds[(960, 540)]
    rgb = [np.ascontiguousarray(np.repeat(grow(a, 4)[:, :, None], 3, axis=2)) for a in small[0]]
    fH, fW = rgb[0].shape[:2]
    pitch = (fW * 3 + 63) // 64 * 64
    keep, ptr = device_planes(rgb, 0, pitch)
    h = lvt_amd.LvtSystem.create(prm, 1)
    assert h.set_pixel_format(lvt_amd.PIX_RGB8) == 0 and h.set_reduction(factor=4, width=fW, height=fH) == 0, h.last_error()
    for it in range(WARM + FRAMES):
        if it == WARM:
            h.profile_enable(True)
        h.track_device_async(ptr[0], ptr[1], fH, fW, pitch)
        h.wait_status()
    out["rgb"] = {"gray_us": slot_us(h, "k_gray_frames"), "reduce_us": slot_us(h, "k_reduce_frames"), "error": h.last_error()}
    print(json.dumps(out))


def p50_and_rate(submit, wait, n_frames):
    """synchronous p50 (us) over FRAMES calls, then frames / s with DEPTH in flight"""
    ts = []
    for i in range(WARM + FRAMES):
        t0 = time.perf_counter()
        submit(i % n_frames); wait()
        ts.append((time.perf_counter() - t0) * 1e6)
    p50 = statistics.median(ts[WARM:])
    inflight, t0 = 0, time.perf_counter()
    for i in range(4 * FRAMES):
        submit(i % n_frames); inflight += 1
        if inflight >= DEPTH:
            wait(); inflight -= 1
    while inflight:
        wait(); inflight -= 1
    return p50, 4 * FRAMES / (time.perf_counter() - t0)


def torch_reduce(t, f):
    """a (H, W) uint8 device tensor -> its block mean, the definition in integer arithmetic"""
    import torch
    H, W = t.shape
    S = t[:H // f * f, :W // f * f].reshape(H // f, f, W // f, f).to(torch.int32).sum(dim=(1, 3))
    return ((S + (f * f) // 2) // (f * f)).to(torch.uint8)


def child_routes(role, sensor):
    """role new: the large frame into a reduced handle; host / torch: the parent's routes (any library)"""
    import torch
    import lvt_amd
    f = 2
    kind, size = ("kitti", (620, 188)) if sensor == 1 else ("tum", (320, 240))
    w, prm, small = world_of(kind, size, 8)
    n = len(small)
    h = lvt_amd.LvtSystem.create(prm, sensor)
    res = {}
    if sensor == 1:
        large = [tuple(grow(a, f) for a in pair) for pair in small]
        fH, fW = large[0][0].shape
        if role == "new":
            assert h.set_reduction(factor=f, width=fW, height=fH) == 0, h.last_error()
            submit = lambda i: h.track_async(*large[i])
        elif role == "host":
            red = host_reducer()
            ring = [None] * (DEPTH + 2)
            t0 = time.perf_counter()
            for _ in range(20):
                red(large[0][0], f)
            res["host_reduce_us_per_image"] = (time.perf_counter() - t0) / 20 * 1e6

            def submit(i, k=[0]):
                ring[k[0] % len(ring)] = pair = (red(large[i][0], f), red(large[i][1], f))   # (alive while in flight)
                k[0] += 1
                h.track_async(*pair)
        else:
            keep, ptr = device_planes([a for pair in large for a in pair], 0, fW)
            views = [torch.as_strided(keep, (fH, fW), (fW, 1), p - keep.data_ptr()) for p in ptr]
            pitch = (size[0] + 63) // 64 * 64
            ring = torch.zeros((DEPTH + 2, 2, size[1], pitch), dtype=torch.uint8, device="cuda")
            ts = torch.cuda.Stream()
            torch.cuda.synchronize()
            h.set_stream(ts.cuda_stream)   # (the caller's stream: the tracker's launches follow the torch kernels in stream order)

            def submit(i, k=[0]):
                r = ring[k[0] % len(ring)]
                k[0] += 1
                with torch.cuda.stream(ts):
                    for e in (0, 1):
                        r[e, :, :size[0]] = torch_reduce(views[2 * i + e], f)
                h.track_device_async(r[0].data_ptr(), r[1].data_ptr(), size[1], size[0], pitch)
        wait = lambda: h.wait_status()
    else:
        large = [(grow(g, f), grow(d.astype(np.float32), f)) for g, d in small]
        fH, fW = large[0][0].shape
        cam = lvt_amd.DepthCamera(width=fW, height=fH, fx=w.fx * f, fy=w.fy * f, cx=(w.cx + 0.5) * f - 0.5, cy=(w.cy + 0.5) * f - 0.5)
        if role == "new":
            assert h.set_reduction(factor=f, width=fW, height=fH) == 0 and h.set_depth_camera(cam) == 0, h.last_error()
            submit = lambda i: h.track_async(*large[i])
        elif role == "host":
            red = host_reducer()
            ring = [None] * (DEPTH + 2)

            def submit(i, k=[0]):
                ring[k[0] % len(ring)] = pair = (red(large[i][0], f), small[i][1])   # (the depth plane at the tracker's size: the caller's own subsampling, not timed)
                k[0] += 1
                h.track_async(*pair)
        else:
            keep, ptr = device_planes([g for g, _ in large], 0, fW)
            views = [torch.as_strided(keep, (fH, fW), (fW, 1), p - keep.data_ptr()) for p in ptr]
            pitch = (size[0] + 63) // 64 * 64
            ring = torch.zeros((DEPTH + 2, size[1], pitch), dtype=torch.uint8, device="cuda")
            depth = torch.from_numpy(np.stack([np.ascontiguousarray(d, dtype=np.float32) for _, d in small])).cuda()
            ts = torch.cuda.Stream()
            torch.cuda.synchronize()
            h.set_stream(ts.cuda_stream)

            def submit(i, k=[0]):
                r = ring[k[0] % len(ring)]
                k[0] += 1
                with torch.cuda.stream(ts):
                    r[:, :size[0]] = torch_reduce(views[i], f)
                h.track_rgbd_device_async(r.data_ptr(), depth[i].data_ptr(), size[1], size[0], pitch, 4 * size[0])
        wait = lambda: h.wait_status()
    res["p50_us"], res["fps"] = p50_and_rate(submit, wait, n)
    res["state"], res["error"] = h.get_state(), h.last_error()
    print(json.dumps(res))


def child_plain():
    """(c) handles that never set the property"""
    import lvt_amd
    res = {}
    w, prm, fr = world_of("kitti", (1241, 376), 8)
    h = lvt_amd.LvtSystem.create(prm, 1)
    res["stereo_async_p50_us"], res["stereo_async_fps"] = p50_and_rate(lambda i: h.track_async(*fr[i]), lambda: h.wait_status(), len(fr))
    h.close()
    h = lvt_amd.LvtSystem.create(prm, 1)
    ts = []
    for i in range(WARM + FRAMES):
        t0 = time.perf_counter()
        h.track(*fr[i % len(fr)])
        ts.append((time.perf_counter() - t0) * 1e6)
    res["lvt_track_p50_us"] = statistics.median(ts[WARM:])
    h.close()
    w, prm, fr = world_of("tum", (640, 480), 8)
    h = lvt_amd.LvtSystem.create(prm, 2)
    ts = []
    for i in range(WARM + FRAMES):
        t0 = time.perf_counter()
        h.track(*fr[i % len(fr)])
        ts.append((time.perf_counter() - t0) * 1e6)
    res["rgbd_track_p50_us"] = statistics.median(ts[WARM:])
    print(json.dumps(res))


def run_child(args, lib=None, limit=300):
    env = dict(os.environ)
    if lib:
        env["LVT_AMD_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit, env=env, cwd=ROOT)
    if out.returncode != 0:
        raise RuntimeError(f"child {args} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    print("done:", " ".join(args), "(parent's library)" if lib else "", file=sys.stderr, flush=True)
    return json.loads(out.stdout.strip().splitlines()[-1])


def fmt(v, nd=1):
    return f"{statistics.median(v):.{nd}f}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="liblvt_c.so of the parent commit, built from a checkout of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_reduction.md"))
    ap.add_argument("--resources", default="", help="the compiler's resource report of k_reduce_frames, for the report")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="new", help=argparse.SUPPRESS)
    ap.add_argument("--sensor", type=int, default=1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == "kernel":
        return child_kernel()
    if a.child == "routes":
        return child_routes(a.role, a.sensor)
    if a.child == "plain":
        return child_plain()
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    kern = [run_child(["--child", "kernel"], limit=500) for _ in range(a.repeats)]
    routes = {(s, r): [] for s in (1, 2) for r in ("new", "host", "torch")}
    plain = {"new": [], "parent": []}
    for _ in range(a.repeats):   # (alternated: this commit's leg, then the parent's)
        for s in (1, 2):
            routes[(s, "new")].append(run_child(["--child", "routes", "--role", "new", "--sensor", str(s)]))
            for r in ("host", "torch"):
                routes[(s, r)].append(run_child(["--child", "routes", "--role", r, "--sensor", str(s)], lib=parent))
        plain["new"].append(run_child(["--child", "plain"]))
        if parent:
            plain["parent"].append(run_child(["--child", "plain"], lib=parent))
    who = "the parent commit's library" if parent else "this commit's library: the parent commit itself was not measured"
    L = ["# Frame reduction: k_reduce_frames measured", "",
         f"One MI355X; medians of {a.repeats} child-process repeats, this commit's legs alternated with the parent's ({who}).  Written by `tools/frame_reduction.py`.",
         "The large frames are small synthetic frames with every pixel repeated f x f times: the tracker tracks them, and the gain of averaging over picking pixels",
         "is NOT what is measured here (that was checked on synthetic texture only, on the CPU oracle; it has not been measured on real footage).", ""]
    if a.resources:
        L += ["Compiler's resource report of `k_reduce_frames`: " + a.resources, ""]
    L += ["## (a) The launch between its HIP events", "",
          "`GB/s` counts the source bytes read plus the destination bytes written.  `copy`: a device-to-device copy of the same source bytes (it reads and writes them: twice the traffic per byte).", "",
          "| Case | Path | us | GB/s | copy us | copy GB/s |", "|---|---|---|---|---|---|"]
    for key in kern[0]:
        if key == "rgb":
            continue
        us = statistics.median([k[key]["us"] for k in kern]); cu = statistics.median([k[key]["copy_us"] for k in kern])
        moved = kern[0][key]["src_bytes"] + kern[0][key]["dst_bytes"]
        name, path = key.split(" | ")
        L.append(f"| {name} | {path} | {us:.1f} | {moved / us / 1e3:.0f} | {cu:.1f} | {2 * kern[0][key]['src_bytes'] / cu / 1e3:.0f} |")
    errs = sorted({k[key]["error"] for k in kern for key in k if k[key]["error"]})
    L += ["", "Reports of the handles: " + (", ".join(errs) if errs else "none") + ".", "",
          "## (b) The parent's routes against this commit's handle", "",
          "`host`: the caller reduces on one core (g++ -O2 restatement), then the gray entry points.  `torch`: the plane is built on the device with torch, then the device entry points on the same stream.", "",
          "| Sensor | Route | synchronous p50 us | frames / s, three in flight |", "|---|---|---|---|"]
    for s in (1, 2):
        for r in ("new", "host", "torch"):
            v = routes[(s, r)]
            L.append(f"| {'stereo 1240 x 376 -> 620 x 188' if s == 1 else 'RGB-D 640 x 480 -> 320 x 240'} | {r} | {fmt([x['p50_us'] for x in v])} | {fmt([x['fps'] for x in v], 0)} |")
    hr = [x.get("host_reduce_us_per_image") for x in routes[(1, "host")] if x.get("host_reduce_us_per_image")]
    if hr:
        L += ["", f"The host restatement over one 1240 x 376 image on one core: {fmt(hr)} us."]
    bad = [(s, r, x["state"], x["error"]) for (s, r), v in routes.items() for x in v if x["state"] != 2 or x["error"]]
    L += ["", "Every leg ended TRACKING without a report." if not bad else f"Legs that did not end TRACKING or left a report: {bad}", "",
          "## (c) Handles that never set the property, against the parent", "",
          "| Route | this commit | spread | parent | spread | verdict |", "|---|---|---|---|---|---|"]
    for key, label in (("stereo_async_fps", "stereo, lvt_amd_track_async, three in flight, frames / s"), ("stereo_async_p50_us", "stereo, lvt_amd_track_async + wait, p50 us"),
                       ("lvt_track_p50_us", "lvt_track p50 us"), ("rgbd_track_p50_us", "lvt_amd_track_rgbd p50 us")):
        nv, pv = [x[key] for x in plain["new"]], [x[key] for x in plain["parent"]]
        if pv:
            inside = abs(statistics.median(nv) - statistics.median(pv)) <= max(max(nv) - min(nv), max(pv) - min(pv))
            L.append(f"| {label} | {fmt(nv)} | {max(nv) - min(nv):.1f} | {fmt(pv)} | {max(pv) - min(pv):.1f} | {'inside the spread of the repeats' if inside else 'OUTSIDE the spread of the repeats'} |")
        else:
            L.append(f"| {label} | {fmt(nv)} | {max(nv) - min(nv):.1f} | not measured | | |")
    g, r = [k["rgb"]["gray_us"] for k in kern], [k["rgb"]["reduce_us"] for k in kern]
    L += ["", "## (d) A 3840 x 2160 RGB8 pair at f = 4: the two launches", "",
          f"`k_gray_frames` {fmt(g)} us (reads 49.8 MB, writes 16.6 MB of gray); `k_reduce_frames` {fmt(r)} us (reads those 16.6 MB, writes 1.0 MB).  A fused kernel would save the",
          "gray write and read, at most the second launch's time plus a quarter of the first's traffic; the decision is left to a later change.", ""]
    open(a.out, "w").write("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    main()
