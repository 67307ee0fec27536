#!/usr/bin/env python3
"""Unregistered depth (lvt_amd_set_depth_camera): the registration inside the feature stage against the route the PARENT commit offered, the caller
registering the depth plane in front of the tracker.  Writes profiles/depth_registration.md.

  host   TUM-shaped RGB-D, 640 x 480 gray + the 16-bit plane of a depth camera 5 cm to the side (focal x 0.9, principal point shifted) at 640 x 480 and at
         320 x 240; pageable host frames: frames/s with three in flight and p50 of the synchronous call.
         new:    a handle with the depth camera fed the sensor's plane (lvt_amd_track_rgbd16[_async]).
         parent: the caller registers on one host core -- a C++ restatement of the definition in include/lvt_amd_ext.h, g++ -O2 -ffp-contract=off, compiled
                 into a helper -- and calls the fp32 entry (lvt_amd_track_rgbd[_async]).  + that registration alone, per frame.
  dev    the same planes resident in HBM, three in flight.  new: the handle reads them in place (lvt_amd_track_rgbd_device_async).
         parent: download (torch, the host waits), the host registration, the fp32 host entry (which uploads).
  klaunch  the two launches as lvt_amd_profile_read reports them (HIP events around each), 100 synchronous frames in every repeat.
  plain  handles that never set a camera, both libraries: the stereo headline route (lvt_amd_track_async, KITTI-shaped) and the TUM-shaped RGB-D route
         (lvt_amd_track_rgbd16_async).  The feature must cost them nothing.

--parent-lib names the PARENT commit's liblvt_c.so, built in a worktree of its own; its legs run in child processes of their own (LVT_AMD_LIB) that
alternate with this library's, three times; every figure is the median of the three (min .. max).  Every child runs under its own time limit, warm-up
first, profiler off (but for klaunch), 300 timed frames; a failing child ends the run (nothing more is started on the GPU).

  python tools/depth_registration.py --parent-lib /path/to/parent/liblvt_c.so [--out profiles/depth_registration.md]
"""
import argparse
import copy
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NREND, WARM, DEPTH, TIMED = 24, 20, 3, 300
SCALE = 1.0 / 5000.0
CAMS = {"640x480": (640, 480), "320x240": (320, 240)}

HOST_REGISTER = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
struct Cam { int w, h; float fx, fy, cx, cy, R[9], t[3]; };
struct Col { float fx, fy, cx, cy, k1, k2, p1, p2, k3; int W, H; };
static inline void proj(const Cam &d, const Col &c, float a, float b, float z, float &u, float &v, float &Zc) {
    const float X = ((a - d.cx) / d.fx) * z, Y = ((b - d.cy) / d.fy) * z;
    const float Xc = (d.R[0] * X + d.R[1] * Y) + d.R[2] * z + d.t[0];
    const float Yc = (d.R[3] * X + d.R[4] * Y) + d.R[5] * z + d.t[1];
    Zc = (d.R[6] * X + d.R[7] * Y) + d.R[8] * z + d.t[2];
    const float x = Xc / Zc, y = Yc / Zc, r2 = x * x + y * y;
    const float rad = 1.f + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
    const float xd = x * rad + (2.f * c.p1 * x * y + c.p2 * (r2 + 2.f * x * x));
    const float yd = y * rad + (c.p1 * (r2 + 2.f * y * y) + 2.f * c.p2 * x * y);
    u = xd * c.fx + c.cx, v = yd * c.fy + c.cy;
}
extern "C" void register_depth16(const Cam *d, const Col *c, const uint16_t *src, float scale, float *dst) {
    const float inf = INFINITY;
    for (long k = 0; k < (long)c->W * c->H; k++) dst[k] = inf;
    for (int j = 0; j < d->h; j++)
        for (int i = 0; i < d->w; i++) {
            const float z = (float)src[(long)j * d->w + i] * scale;
            if (!(z > 0.f && z < inf)) continue;
            float u0, v0, u1, v1, uc, vc, zq, Zc;
            proj(*d, *c, (float)i - 0.5f, (float)j - 0.5f, z, u0, v0, zq);
            proj(*d, *c, (float)i + 0.5f, (float)j + 0.5f, z, u1, v1, zq);
            proj(*d, *c, (float)i, (float)j, z, uc, vc, Zc);
            if (!(Zc > 0.f && Zc < inf)) continue;
            if (!(std::fabs(u0) < 1e6f && std::fabs(v0) < 1e6f && std::fabs(u1) < 1e6f && std::fabs(v1) < 1e6f)) continue;
            int x0 = (int)std::ceil(u0), x1 = (int)std::ceil(u1) - 1, y0 = (int)std::ceil(v0), y1 = (int)std::ceil(v1) - 1;
            if (x1 - x0 >= 16 || y1 - y0 >= 16) continue;
            if (x0 < 0) x0 = 0;
            if (y0 < 0) y0 = 0;
            if (x1 > c->W - 1) x1 = c->W - 1;
            if (y1 > c->H - 1) y1 = c->H - 1;
            for (int y = y0; y <= y1; y++)
                for (int x = x0; x <= x1; x++) {
                    float &o = dst[(long)y * c->W + x];
                    if (Zc < o) o = Zc;
                }
        }
}
"""


class HostCam(C.Structure):
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("R", C.c_float * 9), ("t", C.c_float * 3)]


class HostCol(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")] + [("W", C.c_int), ("H", C.c_int)]


def host_register():
    d = tempfile.mkdtemp(prefix="lvt_depth_reg_")
    src, lib = os.path.join(d, "reg.cpp"), os.path.join(d, "libreg.so")
    with open(src, "w") as f:
        f.write(HOST_REGISTER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src])
    fn = C.CDLL(lib).register_depth16
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    return fn


def pingpong(k):
    p = 2 * (NREND - 1)
    k %= p
    return k if k < NREND else p - k


def camera_spec(prm, w, h, baseline=0.05, focal=0.9, shift=(1.7, -1.3)):
    sx, sy = w / prm.img_width, h / prm.img_height
    return dict(width=w, height=h, fx=prm.fx * sx * focal, fy=prm.fy * sy * focal, cx=prm.cx * sx + shift[0] * sx, cy=prm.cy * sy + shift[1] * sy, t=(baseline, 0.0, 0.0))


def depth_view(world, spec):
    """the world as the depth camera sees it: a shallow copy with the camera's K, size and offset (lvt_amd/synth.py renders eye 1 at `baseline`)"""
    import numpy as np
    d = copy.copy(world)
    d.W, d.H, d.baseline = spec["width"], spec["height"], spec["t"][0]
    d.K = np.array([[spec["fx"], 0, spec["cx"]], [0, spec["fy"], spec["cy"]], [0, 0, 1]], dtype=np.float64)
    d._torch_cache = None
    return d


def tum_frames(lvt, sizes):
    """gray frames (host), and per depth-camera size its 16-bit planes (device tensors, int16 bit patterns)"""
    import torch
    from lvt_amd.synth import make_world
    w = make_world("tum", seed=0)
    prm = lvt.tum_params(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy)
    gray = [w.render_rgbd_torch(i, device="cuda")[0] for i in range(NREND)]
    u16 = {}
    for tag in sizes:
        spec = camera_spec(prm, *CAMS[tag]) if tag != "registered" else None
        v = depth_view(w, spec) if spec else w
        u16[tag] = [torch.clamp(torch.round(v._render_torch(i, (1,) if spec else (0,), "cuda", True)[1].double() * 5000.0), 0, 65535).to(torch.int32).to(torch.int16)
                    for i in range(NREND)]
    torch.cuda.synchronize()
    return w, prm, gray, u16


def timed_async(enq, wait, n):
    import torch
    k = 0
    for _ in range(WARM):
        enq(k); wait(); k += 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    inflight, lost = 0, 0
    for _ in range(n):
        enq(k); k += 1; inflight += 1
        if inflight >= DEPTH:
            lost += wait(); inflight -= 1
    while inflight:
        lost += wait(); inflight -= 1
    torch.cuda.synchronize()
    return round(n / (time.perf_counter() - t0), 1), lost


def timed_sync(call, h):
    k = 0
    for _ in range(WARM):
        call(k); k += 1
    dts = []
    for _ in range(TIMED):
        t0 = time.perf_counter(); call(k); dts.append(time.perf_counter() - t0); k += 1
    return round(1e6 * statistics.median(dts), 1), int(h.get_state() != 2)


def leg(name, role, lvt):
    import numpy as np
    import torch
    out = {}

    def one_wait(h):
        return lambda: int(h.wait_status()[2] != 2)

    if name == "plain":
        from lvt_amd.synth import make_world
        w = make_world("kitti", seed=0)
        prm = lvt.kitti_params(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy, baseline=w.baseline)
        keep = [w.render_stereo_torch(i, device="cuda").cpu().pin_memory() for i in range(NREND)]
        host = [(t[0].numpy(), t[1].numpy()) for t in keep]
        h = lvt.LvtSystem.create(prm, 1)
        fps, lost = timed_async(lambda k: h.track_async(*host[pingpong(k)]), one_wait(h), TIMED)
        out["stereo_async_fps"], out["frames_not_tracking"], out["error"] = fps, lost, h.last_error()
        h.close()
        w, prm, gray, u16 = tum_frames(lvt, ["registered"])
        g = [x.cpu().numpy() for x in gray]
        dep = [u.cpu().numpy().view(np.uint16) for u in u16["registered"]]
        h = lvt.LvtSystem.create(prm, 2)
        fps, lost = timed_async(lambda k: h.track_async(g[pingpong(k)], dep[pingpong(k)], depth_scale=SCALE), one_wait(h), TIMED)
        out["rgbd_async_fps"], out["frames_not_tracking"], out["error"] = fps, out["frames_not_tracking"] + lost, out["error"] + h.last_error()
        h.close()
        return out

    w, prm, gray, u16 = tum_frames(lvt, list(CAMS))
    H, W = w.H, w.W
    g_host = [x.cpu().numpy() for x in gray]
    pitch = (W + 63) // 64 * 64
    g_dev = torch.zeros((NREND, H, pitch), dtype=torch.uint8, device="cuda")
    for i in range(NREND):
        g_dev[i, :, :W] = gray[i]
    reg = host_register() if role == "parent" else None
    col = HostCol(prm.fx, prm.fy, prm.cx, prm.cy, prm.k1, prm.k2, prm.p1, prm.p2, prm.k3, W, H)

    for tag, (dw, dh) in CAMS.items():
        spec = camera_spec(prm, dw, dh)
        dep_host = [u.cpu().numpy().view(np.uint16) for u in u16[tag]]
        hc = HostCam(dw, dh, spec["fx"], spec["fy"], spec["cx"], spec["cy"], (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_float * 3)(*spec["t"]))
        ring = [np.zeros((H, W), np.float32) for _ in range(DEPTH + 2)]    # the parent's route: registered planes, alive while in flight
        down = [torch.zeros((dh, dw), dtype=torch.int16).pin_memory() for _ in range(DEPTH + 2)]

        def make():
            h = lvt.LvtSystem.create(prm, 2)
            if role == "new":
                assert h.set_depth_camera(lvt.DepthCamera(dw, dh, spec["fx"], spec["fy"], spec["cx"], spec["cy"], None, spec["t"])) == 0, h.last_error()
            return h

        def registered(k, src):
            r = ring[k % len(ring)]
            reg(C.byref(hc), C.byref(col), lvt._p(src), SCALE, lvt._p(r))
            return r

        r = {}
        if name == "host":
            h = make()
            if role == "new":
                def enq(k):
                    assert h.track_async(g_host[pingpong(k)], dep_host[pingpong(k)], depth_scale=SCALE) == 0, h.last_error()
                call = lambda k: h.track(g_host[pingpong(k)], dep_host[pingpong(k)], depth_scale=SCALE)   # noqa: E731
            else:
                def enq(k):
                    assert h.track_async(g_host[pingpong(k)], registered(k, dep_host[pingpong(k)])) == 0, h.last_error()
                call = lambda k: h.track(g_host[pingpong(k)], registered(k, dep_host[pingpong(k)]))   # noqa: E731
            fps, lost = timed_async(enq, one_wait(h), TIMED)
            p50, bad = timed_sync(call, h)
            r = dict(async_fps=fps, sync_p50_us=p50, frames_not_tracking=lost + bad, error=h.last_error())
            h.close()
            if role == "parent":
                dts = []
                for k in range(100):
                    t0 = time.perf_counter(); registered(k, dep_host[k % NREND]); dts.append(time.perf_counter() - t0)
                r["host_register_us"] = round(1e6 * statistics.median(dts), 1)
        elif name == "dev":
            h = make()
            if role == "new":
                def enq(k):
                    i = pingpong(k)
                    assert h.track_rgbd_device_async(g_dev[i].data_ptr(), u16[tag][i].data_ptr(), H, W, pitch, 2 * dw, lvt.DEPTH_U16, SCALE) == 0, h.last_error()
            else:
                def enq(k):
                    i, d = pingpong(k), down[k % len(down)]
                    d.copy_(u16[tag][i], non_blocking=True); torch.cuda.current_stream().synchronize()
                    assert h.track_async(g_host[i], registered(k, d.numpy().view(np.uint16))) == 0, h.last_error()
            fps, lost = timed_async(enq, one_wait(h), TIMED)
            r = dict(async_fps=fps, frames_not_tracking=lost, error=h.last_error())
            h.close()
        else:
            assert name == "klaunch" and role == "new"
            h = make()
            for k in range(WARM):
                h.track(g_host[k], dep_host[k], depth_scale=SCALE)
            h.profile_enable(True)
            for k in range(100):
                h.track(g_host[pingpong(WARM + k)], dep_host[pingpong(WARM + k)], depth_scale=SCALE)
            prof = {n: (ms, calls) for n, ms, calls in h.profile_read()}
            r = dict(clear_us=round(1e3 * prof["k_depth_clear"][0] / prof["k_depth_clear"][1], 2),
                     register_us=round(1e3 * prof["k_depth_register"][0] / prof["k_depth_register"][1], 2), calls=prof["k_depth_register"][1],
                     gather_us=round(1e3 * prof["k_gather(+ the rare retry pass)"][0] / prof["k_gather(+ the rare retry pass)"][1], 2), error=h.last_error())
            holes = np.isinf(h.plane(0, 4)[:, :W]).mean()
            r["holes_percent"] = round(100 * float(holes), 2)
            h.close()
        out[tag] = r
    return out


def run_child(args, lib=None, limit=300):
    env = dict(os.environ)
    if lib:
        env["LVT_AMD_LIB"] = lib
    out = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=limit, env=env, cwd=ROOT)
    if out.returncode != 0:   # a failed leg ends the run: nothing more is started on the GPU
        print(json.dumps({"leg": args, "failed": out.returncode, "stderr": out.stderr[-3000:]}), flush=True)
        raise SystemExit(1)
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps({"leg": args[1:], "lib": lib or "this checkout", "result": r}), flush=True)
    return r


def fmt(v, digits=0):
    return f"{statistics.median(v):.{digits}f} ({min(v):.{digits}f} .. {max(v):.{digits}f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="liblvt_c.so of the parent commit, built in a worktree of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_registration.md"))
    ap.add_argument("--resources", default="", help="one line for the report: the kernels' registers and occupancy from the compiler's resource report")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="new", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, ROOT)
        import lvt_amd as lvt
        print(json.dumps({n: leg(n, a.role, lvt) for n in a.child.split(",")}), flush=True)
        return
    me = os.path.abspath(__file__)
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    res = {k: [] for k in ("new", "parent", "plain_new", "plain_parent")}
    for rep in range(3):   # the routes and the two libraries alternate, three times
        res["parent"].append(run_child([me, "--child", "host,dev", "--role", "parent"], lib=parent, limit=420))
        res["new"].append(run_child([me, "--child", "host,dev,klaunch", "--role", "new"], limit=420))
        if parent:
            res["plain_parent"].append(run_child([me, "--child", "plain", "--role", "parent"], lib=parent, limit=420))
        res["plain_new"].append(run_child([me, "--child", "plain", "--role", "parent"], limit=420))

    who = "the parent commit's library" if parent else "this commit's library: the parent commit itself was not measured"
    L = ["# Unregistered depth: registration inside the feature stage", "",
         "Written by `tools/depth_registration.py`.  One synthetic TUM world (640 x 480 gray, seed 0); the depth plane is that of a depth camera 5 cm to the side",
         "(focal x 0.9, principal point shifted by (+1.7, -1.3) px at 640 x 480), 16-bit at 1 / 5000 m, at 640 x 480 and at 320 x 240.",
         "`sync p50`: host clock around the synchronising call, median of 300 calls.  `async`: frames over wall time, 300 frames, three in flight.",
         "Every figure: median of three alternated repeats (min .. max).  `new`: a handle with the depth camera fed the sensor's plane.",
         f"`caller registers`: the parent's route on {who} -- the caller registers on one host core (a C++ restatement of the definition, g++ -O2",
         "-ffp-contract=off) and calls the fp32 entry; planes in HBM are downloaded first (the host waits) and the fp32 host entry uploads the result.", "",
         "| row | depth camera | buffers | new | caller registers | new at least as fast |", "|---|---|---|---|---|---|"]

    def row(title, n, tag, key, lower, unit, where):
        nv, pv = [r[n][tag][key] for r in res["new"]], [r[n][tag][key] for r in res["parent"]]
        bad = sum(r[n][tag]["frames_not_tracking"] for r in res["new"] + res["parent"])
        ok = statistics.median(nv) <= statistics.median(pv) if lower else statistics.median(nv) >= statistics.median(pv)
        d = 1 if lower else 0
        L.append(f"| {title} [{unit}] | {tag} | {where} | {fmt(nv, d)} | {fmt(pv, d)} | {'yes' if ok else 'NO'} |" + (f" frames not tracking: {bad}" if bad else ""))
    for tag in CAMS:
        row("asynchronous, three in flight", "host", tag, "async_fps", False, "frames/s", "host, pageable")
        row("synchronous call, p50", "host", tag, "sync_p50_us", True, "us", "host, pageable")
        row("asynchronous, three in flight", "dev", tag, "async_fps", False, "frames/s", "HBM")
    L.append("")
    for tag in CAMS:
        hv = [r["host"][tag]["host_register_us"] for r in res["parent"]]
        k = {key: [r["klaunch"][tag][key] for r in res["new"]] for key in ("clear_us", "register_us", "gather_us", "holes_percent", "calls")}
        L.append(f"- {tag}: the registration on one host core {fmt(hv, 1)} us per frame; `k_depth_clear` {fmt(k['clear_us'], 2)} us and `k_depth_register` "
                 f"{fmt(k['register_us'], 2)} us per launch as `lvt_amd_profile_read` reports them, each repeat the mean over {k['calls'][0]} synchronous frames (HIP events "
                 f"around each launch: a figure includes the event pair's own few microseconds); `k_gather` behind them {fmt(k['gather_us'], 2)} us; holes in the last "
                 f"registered plane {fmt(k['holes_percent'], 2)} %.")
    L += [f"- compiler's resource report: {a.resources or 'see DESIGN.md'}", "", "## No cost to handles that never set a camera", ""]
    for key, what in (("stereo_async_fps", "stereo headline route, `lvt_amd_track_async`, KITTI-shaped page-locked frames, three in flight [frames/s]"),
                      ("rgbd_async_fps", "TUM-shaped RGB-D, `lvt_amd_track_rgbd16_async`, registered pageable frames, three in flight [frames/s]")):
        nv, pv = [r["plain"][key] for r in res["plain_new"]], [r["plain"][key] for r in res["plain_parent"]]
        line = f"- {what}: this commit {fmt(nv, 1)}, spread {max(nv) - min(nv):.1f}"
        if pv:
            inside = abs(statistics.median(nv) - statistics.median(pv)) <= max(max(pv) - min(pv), max(nv) - min(nv))
            line += f"; parent commit {fmt(pv, 1)}, spread {max(pv) - min(pv):.1f}: the difference of the medians is {'inside' if inside else 'OUTSIDE'} the spread of the repeats" + \
                ("" if inside else f" (this commit is the {'faster' if statistics.median(nv) > statistics.median(pv) else 'SLOWER'} one)")
        else:
            line += "; parent commit: not measured"
        L.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
