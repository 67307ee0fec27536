#!/usr/bin/env python3
"""Depth guard (lvt_amd_set_depth_guard): what the launch costs a guarded handle, what it costs a handle that never sets one (nothing), the only route the
PARENT commit offered -- the caller guarding the depth plane on one host core in front of the tracker --, and what the guard does to a map built from depth
with flying pixels.  Writes profiles/depth_guard.md.

  plain    handles that never set a guard, both libraries: the stereo headline route (lvt_amd_track_async, KITTI-shaped page-locked frames, three in flight),
           the synchronous p50 of lvt_track, the TUM-shaped RGB-D route (lvt_amd_track_rgbd16_async).  The feature must cost them nothing.
  klaunch  k_depth_guard between its HIP events (lvt_amd_profile_read), 100 collected frames of TUM-shaped 640 x 480 16-bit depth: one sequence and a
           lock-step batch of 16, at radius 1 ({1, 4}) and radius 3 ({3, 24}).  One kernel shape was built (a thread per feature).
  rgbd     the same frames.  new: a guarded handle (the default record), 16-bit depth as the sensor delivers it.  plain: the same handle without a guard.
           caller: the caller converts the plane to fp32 metres and zeroes it where the rule drops (a compiled C restatement of the rule over the whole plane,
           one core) and calls the fp32 entry of the parent's library.  Synchronous p50 and frames/s, three in flight.
  effect   the synthetic TUM-shaped sequence with flying pixels planted (a pixel whose 3 x 3 depth range exceeds 0.5 m gets the mean of the window's minimum
           and maximum): the share of map points farther than 5 cm -- along the camera's z, from the nearest of the 3 x 3 ground-truth depths around their
           projection into the last frame -- from their ground-truth surface, and the trajectory error against SynthWorld.pose.  Reported, not asserted.

--parent-lib names the PARENT commit's liblvt_c.so, built in a worktree of its own; its legs run in child processes of their own (LVT_AMD_LIB) that alternate
with this library's, three times; every figure is the median of the three (min .. max).  Every child runs under its own time limit, warm-up first, profiler
off (but for klaunch); a failing child ends the run (nothing more is started on the GPU).

  python tools/depth_guard.py --parent-lib /path/to/parent/liblvt_c.so [--out profiles/depth_guard.md] [--resources "..."]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NREND, WARM, DEPTH, TIMED = 24, 15, 3, 300
SCALE = 1.0 / 5000.0
RECORDS = {1: (1, 4, 0.01, 0.02), 3: (3, 24, 0.01, 0.02)}

# the rule of include/lvt_amd_ext.h, DEPTH GUARD, over a whole 16-bit plane: out = the fp32 conversion, zero where a key point would be dropped
C_RESTATEMENT = r"""
#include <math.h>
void guard_plane(const unsigned short *raw, float scale, int W, int H, int r, int min_support, float tol_abs, float tol_rel, float near_plane, float far_plane,
                 float *s, float *out) {
    for (long i = 0; i < (long)W * H; i++) s[i] = (float)raw[i] * scale;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const float d = s[(long)y * W + x];
            float keep = 0.0f;
            if (near_plane <= d && d <= far_plane) {
                const float t = tol_abs + tol_rel * d;
                int support = 0;
                const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r >= H ? H - 1 : y + r, x0 = x - r < 0 ? 0 : x - r, x1 = x + r >= W ? W - 1 : x + r;
                for (int yy = y0; yy <= y1; yy++)
                    for (int xx = x0; xx <= x1; xx++) {
                        const float v = s[(long)yy * W + xx];
                        support += (near_plane <= v && v <= far_plane && fabsf(v - d) <= t) ? 1 : 0;
                    }
                if (support - 1 >= min_support) keep = d;   /* (the centre counted itself) */
            }
            out[(long)y * W + x] = keep;
        }
}
"""


def pingpong(k):
    p = 2 * (NREND - 1)
    k %= p
    return k if k < NREND else p - k


def compiled_restatement():
    d = tempfile.mkdtemp(prefix="depth_guard_")
    src, so = os.path.join(d, "guard_plane.c"), os.path.join(d, "guard_plane.so")
    with open(src, "w") as f:
        f.write(C_RESTATEMENT)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src, "-lm"])
    fn = ctypes.CDLL(so).guard_plane
    vp, i, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    fn.argtypes, fn.restype = [vp, fl, i, i, i, i, fl, fl, fl, fl, vp, vp], None
    return fn


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


def timed_sync(call, n=TIMED):
    k = 0
    for _ in range(WARM):
        call(k); k += 1
    dts = []
    for _ in range(n):
        t0 = time.perf_counter(); call(k); dts.append(time.perf_counter() - t0); k += 1
    return round(1e6 * statistics.median(dts), 1)


def stereo_world(lvt):
    from lvt_amd.synth import make_world
    w = make_world("kitti", seed=0)
    prm = lvt.kitti_params(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy, baseline=w.baseline)
    keep = [w.render_stereo_torch(i, device="cuda").cpu().pin_memory() for i in range(NREND)]
    return w, prm, keep, [(t[0].numpy(), t[1].numpy()) for t in keep]


def rgbd_world(lvt, n=NREND, f32=False):
    import numpy as np
    import torch
    from lvt_amd.synth import make_world
    w = make_world("tum", seed=0)
    prm = lvt.tum_params(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy)
    fr = []
    for i in range(n):
        g, d = w.render_rgbd_torch(i, device="cuda")
        fr.append((g.cpu().numpy(), d.cpu().numpy() if f32 else torch.clamp(torch.round(d.double() * 5000.0), 0, 65535).to(torch.int32).cpu().numpy().astype(np.uint16)))
    return w, prm, fr


def leg_plain(lvt):
    out = {}
    w, prm, keep, host = stereo_world(lvt)
    h = lvt.LvtSystem.create(prm, 1)
    wait = lambda: int(h.wait_status()[2] != 2)   # noqa: E731
    out["stereo_async_fps"], lost = timed_async(lambda k: h.track_async(*host[pingpong(k)]), wait, TIMED)
    out["stereo_sync_p50_us"] = timed_sync(lambda k: h.track(*host[pingpong(k)]))
    bad, err = lost + int(h.get_state() != 2), h.last_error()
    h.close()
    w, prm, fr = rgbd_world(lvt)
    h = lvt.LvtSystem.create(prm, 2)
    out["rgbd_async_fps"], lost = timed_async(lambda k: h.track_async(*fr[pingpong(k)], depth_scale=SCALE), wait, TIMED)
    out["frames_not_tracking"], out["error"] = bad + lost, err + h.last_error()
    h.close()
    return out


def leg_klaunch(lvt, kind, radius):
    import torch
    w, prm, fr = rgbd_world(lvt)
    cfg = lvt.DepthGuard(*RECORDS[radius])
    if kind == "solo":
        h = lvt.LvtSystem.create(prm, 2)
        assert h.set_depth_guard(cfg) == 0, h.last_error()
        track = lambda k: h.track(*fr[pingpong(k)], depth_scale=SCALE)   # noqa: E731
        state = h.get_state
    else:
        B = 16
        gp = (w.W + 63) // 64 * 64
        dg = torch.zeros((NREND, w.H, gp), dtype=torch.uint8, device="cuda")
        dd = torch.zeros((NREND, w.H, w.W), dtype=torch.int16, device="cuda")
        for i, (g, d) in enumerate(fr):
            dg[i, :, :w.W] = torch.from_numpy(g).cuda()
            dd[i] = torch.from_numpy(d.view("int16")).cuda()
        torch.cuda.synchronize()
        h = lvt.LvtBatch.create_mixed([prm] * B, 2)
        for s in range(B):
            assert h.set_depth_guard(s, cfg) == 0, h.last_error()
        last = []

        def track(k):
            i = pingpong(k)
            rc = h.track_rgbd_device_async([dg[i].data_ptr()] * B, [dd[i].data_ptr()] * B, [w.H] * B, [w.W] * B, [gp] * B, [2 * w.W] * B, lvt.DEPTH_U16, SCALE)
            assert rc == 0, h.last_error()
            last[:] = [h.wait()[2]]
        state = lambda: 2 if (last[0] == 2).all() else 3   # noqa: E731
    for k in range(WARM):
        track(k)
    h.profile_enable(True)
    for k in range(100):
        track(WARM + k)
    prof = {n: (ms, calls) for n, ms, calls in h.profile_read()}
    ms, calls = prof["k_depth_guard"]
    st = h.depth_guard_stats(0) if kind == "batch16" else h.depth_guard_stats()
    out = {"k_depth_guard_us": round(1e3 * ms / max(calls, 1), 2), "calls": calls, "error": h.last_error(), "frames_not_tracking": int(state() != 2),
           "kept": st["kept"], "dropped": st["dropped"]}
    h.close()
    return out


def leg_rgbd(lvt, role):
    import numpy as np
    w, prm, fr = rgbd_world(lvt)
    h = lvt.LvtSystem.create(prm, 2)
    r, ms, ta, tr = RECORDS[1]
    if role == "new":
        assert h.set_depth_guard(lvt.DepthGuard(r, ms, ta, tr)) == 0, h.last_error()
    if role == "caller":
        fn = compiled_restatement()
        ring = [np.zeros((w.H, w.W), np.float32) for _ in range(DEPTH + 2)]   # guarded fp32 planes, alive while in flight
        tmp = np.zeros((w.H, w.W), np.float32)
        near, far = prm.near_plane_distance, prm.far_plane_distance

    def frame(k):
        g, d = fr[pingpong(k)]
        if role != "caller":
            return g, d
        o = ring[k % len(ring)]
        fn(d.ctypes.data, SCALE, w.W, w.H, r, ms, ta, tr, near, far, tmp.ctypes.data, o.ctypes.data)
        return g, o

    def sync(k):
        g, d = frame(k)
        h.track(g, d) if role == "caller" else h.track(g, d, depth_scale=SCALE)

    def enq(k):
        g, d = frame(k)
        rc = h.track_async(g, d) if role == "caller" else h.track_async(g, d, depth_scale=SCALE)
        assert rc == 0, h.last_error()
    out = {"sync_p50_us": timed_sync(sync)}
    bad = int(h.get_state() != 2)
    out["async_fps"], lost = timed_async(enq, lambda: int(h.wait_status()[2] != 2), TIMED)
    out["frames_not_tracking"], out["error"] = bad + lost, h.last_error()
    out["n_left"] = h.counts()["n_left"]
    h.close()
    if role == "caller":
        dts = []
        for k in range(50):
            t0 = time.perf_counter(); frame(k); dts.append(time.perf_counter() - t0)
        out["host_guard_us_per_frame"] = round(1e6 * statistics.median(dts), 1)
    return out


def plant_flying_pixels(d):
    """a pixel whose 3 x 3 depth range exceeds 0.5 m gets the mean of the window's minimum and maximum; returns (plane, share of pixels planted)"""
    import numpy as np
    H, W = d.shape
    p = np.pad(d, 1, mode="edge")
    win = np.stack([p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    lo, hi = win.min(0), win.max(0)
    on = hi - lo > np.float32(0.5)
    return np.where(on, ((lo + hi) * np.float32(0.5)).astype(np.float32), d).astype(np.float32), float(on.mean())


def leg_effect(lvt, n=60):
    import numpy as np
    w, prm, fr = rgbd_world(lvt, n, f32=True)
    planted = [plant_flying_pixels(d) for _, d in fr]
    rows = {}
    for name, planes, rec in (("clean depth, no guard", [d for _, d in fr], None), ("flying pixels, no guard", [p for p, _ in planted], None),
                              ("flying pixels, default guard {1, 4, 0.01, 0.02}", [p for p, _ in planted], (1, 4, 0.01, 0.02)),
                              ("flying pixels, guard {1, 6, 0.01, 0.02}", [p for p, _ in planted], (1, 6, 0.01, 0.02))):
        h = lvt.LvtSystem.create(prm, 2)
        if rec:
            assert h.set_depth_guard(lvt.DepthGuard(*rec)) == 0, h.last_error()
        errs, lost, dropped = [], 0, 0
        for i in range(n):
            R, t = h.track(fr[i][0], planes[i])
            lost += int(h.get_state() != 2)
            errs.append(float(np.linalg.norm(np.asarray(t) - w.pose(i)[1])))
            if rec:
                dropped += h.depth_guard_stats()["dropped"]
        xyz = h.map()[0]
        pc = (xyz - np.asarray(t)) @ np.asarray(R).reshape(3, 3)      # R^T (p - t): the map in the last camera's frame, by the tracker's own pose
        z = np.where(pc[:, 2] > 0, pc[:, 2], 1.0)
        iu, iv = np.rint(prm.fx * pc[:, 0] / z + prm.cx).astype(int), np.rint(prm.fy * pc[:, 1] / z + prm.cy).astype(int)
        ok = (pc[:, 2] > 0) & (iu >= 1) & (iu < w.W - 1) & (iv >= 1) & (iv < w.H - 1)
        truth = np.pad(fr[n - 1][1], 1, mode="edge")
        win = np.stack([truth[dy:dy + w.H, dx:dx + w.W] for dy in range(3) for dx in range(3)])
        dist = np.abs(win[:, iv[ok], iu[ok]] - pc[ok, 2]).min(0)
        rows[name] = {"map_points": int(len(xyz)), "in_view": int(ok.sum()), "share_off_5cm": round(float((dist > 0.05).mean()), 4),
                      "traj_rmse_mm": round(1e3 * float(np.sqrt(np.mean(np.square(errs)))), 3), "traj_max_mm": round(1e3 * max(errs), 3),
                      "frames_not_tracking": lost, "dropped_per_frame": round(dropped / n, 1), "error": h.last_error()}
        h.close()
    return {"rows": rows, "planted_share": round(statistics.mean(s for _, s in planted), 4), "frames": n}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_guard.md"))
    ap.add_argument("--resources", default="", help="the compiler's resource report of the kernel, for the report")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="new", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, ROOT)
        import lvt_amd as lvt
        what, _, kind = a.child.partition(":")
        if what == "klaunch":
            shape, _, radius = kind.partition(":")
            r = leg_klaunch(lvt, shape, int(radius))
        else:
            r = leg_rgbd(lvt, a.role) if what == "rgbd" else leg_effect(lvt) if what == "effect" else leg_plain(lvt)
        print(json.dumps(r), flush=True)
        return
    me = os.path.abspath(__file__)
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    plain = {"new": [], "parent": []}
    rgbd = {"new": [], "plain": [], "caller": []}
    kinds = ("solo:1", "solo:3", "batch16:1", "batch16:3")
    kl = {k: [] for k in kinds}
    for rep in range(a.repeats):   # the two libraries alternate
        if parent:
            plain["parent"].append(run_child([me, "--child", "plain"], lib=parent))
        plain["new"].append(run_child([me, "--child", "plain"]))
        rgbd["caller"].append(run_child([me, "--child", "rgbd", "--role", "caller"], lib=parent))
        rgbd["new"].append(run_child([me, "--child", "rgbd", "--role", "new"]))
        rgbd["plain"].append(run_child([me, "--child", "rgbd", "--role", "plain"]))
        for k in kinds:
            kl[k].append(run_child([me, "--child", "klaunch:" + k]))
    effect = run_child([me, "--child", "effect"])

    who = "the parent commit's library" if parent else "this commit's library: the parent commit itself was not measured"
    L = ["# Depth guard: RGB-D key points whose depth has no support dropped inside the feature stage", "",
         "Written by `tools/depth_guard.py`.  Synthetic worlds (seed 0) of KITTI (1241 x 376 stereo) and TUM (640 x 480 RGB-D, 16-bit depth) shape.",
         f"`sync p50`: host clock around the synchronising call, median of {TIMED} calls.  `async`: frames over wall time, {TIMED} frames, three in flight.",
         f"Every figure: median of {a.repeats} alternated repeats in child processes of their own (min .. max).", "",
         "## No cost to handles that never set a guard", ""]
    for key, what, lower in (("stereo_async_fps", "stereo headline route, `lvt_amd_track_async`, KITTI-shaped page-locked frames, three in flight [frames/s]", False),
                             ("stereo_sync_p50_us", "`lvt_track`, KITTI-shaped, synchronous p50 [us]", True),
                             ("rgbd_async_fps", "TUM-shaped RGB-D, `lvt_amd_track_rgbd16_async`, pageable frames, three in flight [frames/s]", False)):
        nv, pv = [r[key] for r in plain["new"]], [r[key] for r in plain["parent"]]
        line = f"- {what}: this commit {fmt(nv, 1)}, spread {max(nv) - min(nv):.1f}"
        if pv:
            inside = abs(statistics.median(nv) - statistics.median(pv)) <= max(max(pv) - min(pv), max(nv) - min(nv))
            faster = (statistics.median(nv) < statistics.median(pv)) == lower
            line += f"; parent commit {fmt(pv, 1)}, spread {max(pv) - min(pv):.1f}: the difference of the medians is {'inside' if inside else 'OUTSIDE'} the spread of the repeats" + \
                    ("" if inside else f" (this commit is the {'faster' if faster else 'SLOWER'} one)")
        else:
            line += "; parent commit: not measured"
        L.append(line)
    bad = sum(r["frames_not_tracking"] for r in plain["new"] + plain["parent"])
    L += ([f"- frames not tracking: {bad}"] if bad else []) + ["", "## The launch", "",
          "`k_depth_guard` between its HIP events, as `lvt_amd_profile_read` reports it (the figure includes the event pair's own few microseconds), mean over 100",
          "collected frames per repeat.  One workgroup of 1024 threads per sequence, a thread per feature: the one kernel shape that was built (the shape with a",
          "few lanes per feature and a cross-lane sum was not built, so it was not measured).", "",
          "| handle | record | k_depth_guard [us] | kept / dropped, last frame |", "|---|---|---|---|"]
    names = {"solo": "one TUM-shaped RGB-D sequence", "batch16": "lock-step batch of 16 TUM-shaped sequences, every sequence guarded"}
    for k in kinds:
        shape, _, radius = k.partition(":")
        r = kl[k][-1]
        L.append(f"| {names[shape]} | {{{', '.join(str(x) for x in RECORDS[int(radius)])}}} | {fmt([x['k_depth_guard_us'] for x in kl[k]], 2)} | {r['kept']} / {r['dropped']} |")
    L += ["", f"- compiler's resource report: {a.resources or 'see DESIGN.md'}", "", "## The guard inside the tracker against the caller guarding the plane", "",
          "`guarded`: a handle with the default record, fed the 16-bit depth plane as the sensor delivers it.  `unguarded`: the same frames, no guard.  `caller guards`:",
          "the only route the parent has, on " + who + " -- the caller converts the plane to fp32 metres and zeroes it where the rule drops (a compiled C restatement",
          "over the whole plane, `cc -O2`, one host core), then calls the fp32 entry.", "",
          "| row | guarded | unguarded | caller guards | guarded at least as fast as the caller |", "|---|---|---|---|---|"]
    for key, title, lower in (("sync_p50_us", "synchronous p50 [us]", True), ("async_fps", "host frames, three in flight [frames/s]", False)):
        nv, uv, pv = ([r[key] for r in rgbd[k]] for k in ("new", "plain", "caller"))
        ok = statistics.median(nv) <= statistics.median(pv) if lower else statistics.median(nv) >= statistics.median(pv)
        L.append(f"| {title} | {fmt(nv, 1)} | {fmt(uv, 1)} | {fmt(pv, 1)} | {'yes' if ok else 'NO'} |")
    bad = sum(r["frames_not_tracking"] for k in rgbd for r in rgbd[k])
    same = {r["n_left"] for r in rgbd["new"]} == {r["n_left"] for r in rgbd["caller"]}
    L += ["", f"- the caller's conversion and guarding of one 640 x 480 plane on one core: {fmt([r['host_guard_us_per_frame'] for r in rgbd['caller']], 1)} us.",
          f"- the guarded handle and the caller's route end their last frame with {'the same' if same else 'DIFFERENT'} feature count; frames not tracking: {bad}.", "",
          "## Effect on a map built from depth with flying pixels", "",
          f"{effect['frames']} frames of the TUM-shaped world; a pixel whose 3 x 3 depth range exceeds 0.5 m gets the mean of the window's minimum and maximum",
          f"({100 * effect['planted_share']:.1f} % of the pixels).  A map point is `off` when, brought into the last camera's frame by the tracker's own pose and projected, its z",
          "differs by more than 5 cm from every one of the 3 x 3 ground-truth depths around its pixel.  Trajectory error: position against `SynthWorld.pose`.",
          "Reported, not asserted: one run, no repeats.", "",
          "| run | map points (in view) | off by more than 5 cm | trajectory RMSE / max [mm] | dropped per frame | frames not tracking |", "|---|---|---|---|---|---|"]
    for name, r in effect["rows"].items():
        L.append(f"| {name} | {r['map_points']} ({r['in_view']}) | {100 * r['share_off_5cm']:.2f} % | {r['traj_rmse_mm']:.2f} / {r['traj_max_mm']:.2f} | {r['dropped_per_frame']} | {r['frames_not_tracking']} |")
    L += ["", "The planted pixels form a band two pixels wide along every layer edge, and both pixels of the band carry the same in-between depth: a flying pixel has up",
          "to five neighbours that agree with it: a record that asks for four can be met inside the band, {1, 6} asks for more than the band alone can give."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
