#!/usr/bin/env python3
"""Colour frames (lvt_amd_set_pixel_format): the conversion to gray inside the feature stage against the route the PARENT commit offered, the caller
converting in front of the tracker.  Writes profiles/colour_frames.md.

  rgbd_host   TUM-shaped RGB-D (640 x 480, RGB8 + 16-bit depth), host frames, pageable and page-locked: frames/s with three in flight
              (lvt_amd_track_rgbd16_async) and p50 of the synchronous call (lvt_amd_track_rgbd16).
              new:    a colour handle fed the RGB frames.
              parent: examples/image_io.h: to_gray over the frame on the host -- the example's own C++ loop, compiled into a helper -- then the gray entry.
              gray:   the same sequence as gray frames through a gray handle: what colour costs over gray (3x the bytes over PCIe, one more launch).
              + the host conversion alone, per frame, on one core.
  rgbd_dev    colour planes resident in HBM, three in flight.  new: the colour handle reads them in place (lvt_amd_track_rgbd_device_async).
              caller: a torch integer expression into a pitched gray plane on the caller's stream, an event the host waits for (this leg's handle keeps its
              private streams, which are ordered behind nothing of the caller's; lvt_amd_set_stream would order it behind the caller's stream without the
              host wait, at the price of the feature stage's overlap), then the same call on a gray handle.
  kgray       the k_gray_frames launch as lvt_amd_profile_read reports it (HIP events around the launch), 100 synchronous frames.
  plain       handles that never set a format, both libraries: the stereo headline route (lvt_amd_track_async, KITTI-shaped) and the TUM-shaped RGB-D
              route (lvt_amd_track_rgbd16_async, gray).  The feature must cost them nothing.

--parent-lib names the PARENT commit's liblvt_c.so, built in a worktree of its own; its legs run in child processes of their own (LVT_AMD_LIB) that
alternate with this library's, three times; every figure is the median of the three (min .. max).  Every child runs under its own time limit, warm-up
first, profiler off (but for kgray), 300 timed frames; a failing child ends the run (nothing more is started on the GPU).

  python tools/colour_frames.py --parent-lib /path/to/parent/liblvt_c.so [--out profiles/colour_frames.md]
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

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NREND, WARM, DEPTH, TIMED = 40, 20, 3, 300
SCALE = 1.0 / 5000.0
PIX_RGB8 = 2


def pingpong(k):
    p = 2 * (NREND - 1)
    k %= p
    return k if k < NREND else p - k


def host_converter():
    """examples/image_io.h: to_gray over an interleaved RGB frame, compiled as the examples are (g++ -O2)"""
    d = tempfile.mkdtemp(prefix="lvt_to_gray_")
    src, lib = os.path.join(d, "to_gray.cpp"), os.path.join(d, "libto_gray.so")
    with open(src, "w") as f:
        f.write('#include "image_io.h"\nextern "C" void rgb_to_gray(const unsigned char *rgb, unsigned char *gray, long n) {\n'
                "    for (long i = 0; i < n; i++) gray[i] = lvt_io::to_gray(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);\n}\n")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "examples"), "-o", lib, src])
    fn = C.CDLL(lib).rgb_to_gray
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    return fn


def colourise(gray, gen):
    """(H, W) uint8 tensor -> (H, W, 3) RGB: every channel the gray value plus integer noise of its own amplitude"""
    import torch
    g = gray.to(torch.int16)
    ch = [torch.clamp(g + torch.randint(-a, a + 1, g.shape, generator=gen, device=g.device, dtype=torch.int16), 0, 255).to(torch.uint8) for a in (24, 8, 32)]
    return torch.stack(ch, dim=2).contiguous()


def torch_gray(rgb, out):
    """the caller's own GPU conversion: the formula as a torch integer expression, written into the pitched plane `out`"""
    import torch
    v = rgb.to(torch.int32)
    out[:, :rgb.shape[1]] = ((v[:, :, 0] * 4899 + v[:, :, 1] * 9617 + v[:, :, 2] * 1868 + 8192) >> 14).to(torch.uint8)


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
    return dict(sync_p50_us=round(1e6 * statistics.median(dts), 1), frames_not_tracking=int(h.get_state() != 2), error=h.last_error())


def tum_frames(lvt):
    import torch
    from lvt_amd.synth import make_world
    w = make_world("tum", seed=0)
    prm = lvt.tum_params(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy)
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    rgb, u16 = [], []
    for i in range(NREND):
        g, d = w.render_rgbd_torch(i, device="cuda")
        rgb.append(colourise(g, gen))
        u16.append(torch.clamp(torch.round(d.double() * 5000.0), 0, 65535).to(torch.int32))
    torch.cuda.synchronize()
    return w, prm, rgb, u16


def leg(name, role, lvt):
    """role: "new" (a colour handle), "parent" (the caller converts in front of a gray handle), "gray" (gray frames, a gray handle)"""
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
        w, prm, rgb, u16 = tum_frames(lvt)
        gray = [np.ascontiguousarray(((r.to(torch.int32) * torch.tensor([4899, 9617, 1868], device="cuda", dtype=torch.int32)).sum(2) + 8192 >> 14).to(torch.uint8).cpu().numpy()) for r in rgb]
        dep = [u.cpu().numpy().astype(np.uint16) for u in u16]
        h = lvt.LvtSystem.create(prm, 2)
        fps, lost = timed_async(lambda k: h.track_async(gray[pingpong(k)], dep[pingpong(k)], depth_scale=SCALE), one_wait(h), TIMED)
        out["rgbd_async_fps"], out["frames_not_tracking"], out["error"] = fps, out["frames_not_tracking"] + lost, out["error"] + h.last_error()
        h.close()
        return out

    w, prm, rgb, u16 = tum_frames(lvt)
    H, W = w.H, w.W
    pitch = (W + 63) // 64 * 64

    if name == "rgbd_host":
        conv = host_converter()
        for pin in (False, True):
            mk = (lambda t: t.cpu().pin_memory()) if pin else (lambda t: t.cpu())
            keep = [(mk(r), mk(u.to(torch.int16))) for r, u in zip(rgb, u16)]
            col = [a.numpy() for a, _ in keep]
            dep = [b.numpy().view(np.uint16) for _, b in keep]
            gkeep = [mk(torch.zeros((H, W), dtype=torch.uint8)) for _ in range(NREND)]
            gray = [g.numpy() for g in gkeep]
            for c, g in zip(col, gray):
                conv(lvt._p(c), lvt._p(g), H * W)
            ring = [mk(torch.zeros((H, W), dtype=torch.uint8)).numpy() for _ in range(DEPTH + 2)]   # the parent's route: converted frames, alive while in flight
            tag = "pinned" if pin else "pageable"
            h = lvt.LvtSystem.create(prm, 2)
            if role == "new":
                assert h.set_pixel_format(PIX_RGB8) == 0, h.last_error()

            def frame(k):
                i = pingpong(k)
                if role == "new":
                    return col[i], dep[i]
                if role == "gray":
                    return gray[i], dep[i]
                g = ring[k % len(ring)]
                conv(lvt._p(col[i]), lvt._p(g), H * W)
                return g, dep[i]

            def enq(k):
                a, d = frame(k)
                assert h.track_async(a, d, depth_scale=SCALE) == 0, h.last_error()
            fps, lost = timed_async(enq, one_wait(h), TIMED)
            r = timed_sync(lambda k: h.track(*frame(k), depth_scale=SCALE), h)
            r.update(async_fps=fps, frames_not_tracking=r["frames_not_tracking"] + lost)
            out[tag] = r
            h.close()
        dts = []
        for k in range(TIMED):
            t0 = time.perf_counter(); conv(lvt._p(col[k % NREND]), lvt._p(ring[0]), H * W); dts.append(time.perf_counter() - t0)
        out["to_gray_us"] = round(1e6 * statistics.median(dts), 1)
        return out

    if name == "rgbd_dev":
        dep = [u.to(torch.int16) for u in u16]
        h = lvt.LvtSystem.create(prm, 2)
        if role == "new":
            assert h.set_pixel_format(PIX_RGB8) == 0, h.last_error()

            def enq(k):
                i = pingpong(k)
                assert h.track_rgbd_device_async(rgb[i].data_ptr(), dep[i].data_ptr(), H, W, 3 * W, 2 * W, lvt.DEPTH_U16, SCALE) == 0, h.last_error()
        else:
            stream, ev = torch.cuda.Stream(), torch.cuda.Event()
            ring = torch.zeros((DEPTH + 2, H, pitch), dtype=torch.uint8, device="cuda")

            def enq(k):
                i, dst = pingpong(k), ring[k % len(ring)]
                with torch.cuda.stream(stream):
                    torch_gray(rgb[i], dst)
                ev.record(stream); ev.synchronize()
                assert h.track_rgbd_device_async(dst.data_ptr(), dep[i].data_ptr(), H, W, pitch, 2 * W, lvt.DEPTH_U16, SCALE) == 0, h.last_error()
        fps, lost = timed_async(enq, one_wait(h), TIMED)
        err = h.last_error()
        h.close()
        return dict(async_fps=fps, frames_not_tracking=lost, error=err)

    assert name == "kgray"
    h = lvt.LvtSystem.create(prm, 2)
    assert h.set_pixel_format(PIX_RGB8) == 0, h.last_error()
    col = [r.cpu().numpy() for r in rgb]
    dep = [u.cpu().numpy().astype(np.uint16) for u in u16]
    for k in range(WARM):
        h.track(col[k], dep[k], depth_scale=SCALE)
    h.profile_enable(True)
    for k in range(100):
        h.track(col[pingpong(WARM + k)], dep[pingpong(WARM + k)], depth_scale=SCALE)
    prof = {n: (ms, calls) for n, ms, calls in h.profile_read()}
    ms, calls = prof["k_gray_frames"]
    err = h.last_error()
    h.close()
    return dict(k_gray_frames_us=round(1e3 * ms / max(calls, 1), 2), calls=calls, error=err)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_frames.md"))
    ap.add_argument("--resources", default="", help="one line for the report: k_gray_frames' registers and occupancy from the compiler's resource report")
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
    res = {k: [] for k in ("new", "parent", "gray", "plain_new", "plain_parent")}
    for rep in range(3):   # the routes and the two libraries alternate, three times
        res["parent"].append(run_child([me, "--child", "rgbd_host,rgbd_dev", "--role", "parent"], lib=parent, limit=420))
        res["new"].append(run_child([me, "--child", "rgbd_host,rgbd_dev" + (",kgray" if rep == 0 else ""), "--role", "new"], limit=420))
        res["gray"].append(run_child([me, "--child", "rgbd_host", "--role", "gray"], limit=420))
        if parent:
            res["plain_parent"].append(run_child([me, "--child", "plain", "--role", "gray"], lib=parent, limit=420))
        res["plain_new"].append(run_child([me, "--child", "plain", "--role", "gray"], limit=420))

    who = "the parent commit's library" if parent else "this commit's library: the parent commit itself was not measured"
    kg = res["new"][0]["kgray"]
    L = ["# Colour frames: gray conversion inside the feature stage", "",
         "Written by `tools/colour_frames.py`.  One synthetic TUM world (640 x 480, seed 0), colourised (every channel the gray value plus noise of its own), RGB8 + 16-bit depth.",
         "`sync p50`: host clock around the synchronising call, median of 300 calls.  `async`: frames over wall time, 300 frames, three in flight.",
         "Every figure: median of three alternated repeats (min .. max).  `new`: a handle with LVT_AMD_PIX_RGB8 fed the colour frames.",
         f"`caller converts`: the parent's route on {who} -- host frames through `examples/image_io.h: to_gray` (the example's C++ loop, g++ -O2, one core),",
         "planes in HBM through a torch integer expression on the caller's stream plus an event the host waits for -- then the gray entry point.",
         "`gray`: the same sequence as gray frames through a gray handle of this commit: what colour costs over gray.", "",
         "| row | buffers | new | caller converts | gray | new at least as fast as the caller's conversion |", "|---|---|---|---|---|---|"]

    def row(title, n, tag, key, lower, unit):
        pick = (lambda r: r[n][tag][key]) if tag else (lambda r: r[n][key])
        nv, pv = [pick(r) for r in res["new"]], [pick(r) for r in res["parent"]]
        gv = [pick(r) for r in res["gray"]] if n == "rgbd_host" else None
        bad = sum((r[n][tag] if tag else r[n])["frames_not_tracking"] for r in res["new"] + res["parent"])
        ok = statistics.median(nv) <= statistics.median(pv) if lower else statistics.median(nv) >= statistics.median(pv)
        d = 1 if lower else 0
        L.append(f"| {title} [{unit}] | {tag or 'HBM'} | {fmt(nv, d)} | {fmt(pv, d)} | {fmt(gv, d) if gv else '-'} | {'yes' if ok else 'NO'} |" + (f" frames not tracking: {bad}" if bad else ""))
    for tag in ("pageable", "pinned"):
        row("RGB-D host frames, asynchronous", "rgbd_host", tag, "async_fps", False, "frames/s")
        row("RGB-D host frames, synchronous p50", "rgbd_host", tag, "sync_p50_us", True, "us")
    row("RGB-D planes in HBM, asynchronous", "rgbd_dev", None, "async_fps", False, "frames/s")
    tg = [r["rgbd_host"]["to_gray_us"] for r in res["parent"] + res["new"] + res["gray"]]
    L += ["", f"- `to_gray` over one 640 x 480 RGB frame on one host core: {fmt(tg, 1)} us.",
          f"- `k_gray_frames` (one 640 x 480 RGB8 image) as `lvt_amd_profile_read` reports it: {kg['k_gray_frames_us']} us per launch over {kg['calls']} frames (HIP events around the launch: the figure includes the event pair's own few microseconds).",
          f"- compiler's resource report for `k_gray_frames`: {a.resources or 'see DESIGN.md'}", "", "## No cost to handles that never set a format", ""]
    for key, what in (("stereo_async_fps", "stereo headline route, `lvt_amd_track_async`, KITTI-shaped page-locked frames, three in flight [frames/s]"),
                      ("rgbd_async_fps", "TUM-shaped RGB-D, `lvt_amd_track_rgbd16_async`, gray pageable frames, three in flight [frames/s]")):
        nv, pv = [r["plain"][key] for r in res["plain_new"]], [r["plain"][key] for r in res["plain_parent"]]
        line = f"- {what}: this commit {fmt(nv, 1)}, spread {max(nv) - min(nv):.1f}"
        if pv:
            inside = abs(statistics.median(nv) - statistics.median(pv)) <= max(pv) - min(pv)
            line += f"; parent commit {fmt(pv, 1)}, spread {max(pv) - min(pv):.1f}: the difference of the medians is {'inside' if inside else 'OUTSIDE'} the parent's own spread" + ("" if inside else f" (this commit is the {'faster' if statistics.median(nv) > statistics.median(pv) else 'SLOWER'} one)")
        else:
            line += "; parent commit: not measured"
        L.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
