#!/usr/bin/env python3
"""Feature masks (lvt_amd_set_mask): what the launch costs a masked handle, what it costs a handle that never sets one (nothing), and -- for RGB-D -- the only
route the PARENT commit offered, the caller zeroing depth under the mask on one host core in front of the tracker.  Writes profiles/feature_masks.md.

  plain    handles that never set a mask, both libraries: the stereo headline route (lvt_amd_track_async, KITTI-shaped page-locked frames, three in flight),
           the synchronous p50 of lvt_track, the TUM-shaped RGB-D route (lvt_amd_track_rgbd16_async).  The feature must cost them nothing.
  klaunch  k_mask_features between its HIP events (lvt_amd_profile_read), 100 collected frames: a KITTI-shaped pair (1241 x 376, both eyes masked), a
           TUM-shaped image (640 x 480) and a lock-step batch of 16 KITTI-shaped pairs (every sequence masked), under the bonnet mask (rows below 0.7 H zero).
  rgbd     TUM-shaped RGB-D under the bonnet mask.  new: a masked handle, 16-bit depth as the sensor delivers it.  parent: the caller converts the depth to fp32
           metres with zeros under the mask (numpy, one core) and calls the fp32 entry of the parent's library.  Synchronous p50 and frames/s, three in flight.
           Stereo has no route on the parent commit short of the caller running its own detector, so no stereo comparison is made.

--parent-lib names the PARENT commit's liblvt_c.so, built in a worktree of its own; its legs run in child processes of their own (LVT_AMD_LIB) that alternate
with this library's, three times; every figure is the median of the three (min .. max).  Every child runs under its own time limit, warm-up first, profiler
off (but for klaunch); a failing child ends the run (nothing more is started on the GPU).

  python tools/feature_masks.py --parent-lib /path/to/parent/liblvt_c.so [--out profiles/feature_masks.md] [--resources "..."]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NREND, WARM, DEPTH, TIMED = 24, 15, 3, 300
SCALE = 1.0 / 5000.0


def pingpong(k):
    p = 2 * (NREND - 1)
    k %= p
    return k if k < NREND else p - k


def bonnet(W, H):
    import numpy as np
    m = np.full((H, W), 255, np.uint8)
    m[int(0.7 * H):] = 0
    return m


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


def rgbd_world(lvt):
    import numpy as np
    import torch
    from lvt_amd.synth import make_world
    w = make_world("tum", seed=0)
    prm = lvt.tum_params(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy)
    fr = []
    for i in range(NREND):
        g, d = w.render_rgbd_torch(i, device="cuda")
        fr.append((g.cpu().numpy(), torch.clamp(torch.round(d.double() * 5000.0), 0, 65535).to(torch.int32).cpu().numpy().astype(np.uint16)))
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


def mask_row(h):
    prof = {n: (ms, calls) for n, ms, calls in h.profile_read()}
    ms, calls = prof["k_mask_features"]
    return {"k_mask_features_us": round(1e3 * ms / max(calls, 1), 2), "calls": calls}


def leg_klaunch(lvt, kind):
    import torch
    if kind == "tum":
        w, prm, fr = rgbd_world(lvt)
        h = lvt.LvtSystem.create(prm, 2)
        assert h.set_mask(bonnet(w.W, w.H)) == 0, h.last_error()
        track = lambda k: h.track(*fr[pingpong(k)], depth_scale=SCALE)   # noqa: E731
        state = h.get_state
    elif kind == "kitti":
        w, prm, keep, host = stereo_world(lvt)
        h = lvt.LvtSystem.create(prm, 1)
        assert h.set_mask(bonnet(w.W, w.H), bonnet(w.W, w.H)) == 0, h.last_error()
        track = lambda k: h.track(*host[pingpong(k)])   # noqa: E731
        state = h.get_state
    else:
        B = 16
        w, prm, keep, host = stereo_world(lvt)
        pitch = (w.W + 63) // 64 * 64
        dev = torch.zeros((NREND, 2, w.H, pitch), dtype=torch.uint8, device="cuda")
        for i, t in enumerate(keep):
            dev[i, :, :, :w.W] = t.cuda()
        torch.cuda.synchronize()
        h = lvt.LvtBatch(prm, B)
        for s in range(B):
            assert h.set_mask(s, bonnet(w.W, w.H), bonnet(w.W, w.H)) == 0, h.last_error()
        last = []

        def track(k):
            i = pingpong(k)
            h.track_device_async([dev[i, 0].data_ptr()] * B, [dev[i, 1].data_ptr()] * B, w.H, w.W, pitch)
            last[:] = [h.wait()[2]]
        state = lambda: 2 if (last[0] == 2).all() else 3   # noqa: E731
    for k in range(WARM):
        track(k)
    h.profile_enable(True)
    for k in range(100):
        track(WARM + k)
    out = mask_row(h)
    st = h.mask_stats(0) if kind == "batch16" else h.mask_stats()
    out.update(error=h.last_error(), frames_not_tracking=int(state() != 2), kept=list(st["kept"]), dropped=list(st["dropped"]))
    h.close()
    return out


def leg_rgbd(lvt, role):
    import numpy as np
    w, prm, fr = rgbd_world(lvt)
    mask = bonnet(w.W, w.H)
    new = role == "new"
    h = lvt.LvtSystem.create(prm, 2)
    if new:
        assert h.set_mask(mask) == 0, h.last_error()
    ring = [np.zeros((w.H, w.W), np.float32) for _ in range(DEPTH + 2)]   # the parent's route: masked fp32 planes, alive while in flight
    on = mask != 0
    scale = np.float32(SCALE)

    def frame(k):
        g, d = fr[pingpong(k)]
        if new:
            return g, d
        r = ring[k % len(ring)]
        np.multiply(d, scale, out=r, dtype=np.float32)   # one core: the conversion the caller needs for the fp32 entry ...
        np.multiply(r, on, out=r)                        # ... and the zeros under the mask
        return g, r

    def sync(k):
        g, d = frame(k)
        h.track(g, d, depth_scale=SCALE) if new else h.track(g, d)

    def enq(k):
        g, d = frame(k)
        rc = h.track_async(g, d, depth_scale=SCALE) if new else h.track_async(g, d)
        assert rc == 0, h.last_error()
    out = {"sync_p50_us": timed_sync(sync)}
    bad = int(h.get_state() != 2)
    out["async_fps"], lost = timed_async(enq, lambda: int(h.wait_status()[2] != 2), TIMED)
    out["frames_not_tracking"], out["error"] = bad + lost, h.last_error()
    out["n_left"] = h.counts()["n_left"]
    h.close()
    if not new:
        dts = []
        for k in range(50):
            t0 = time.perf_counter(); frame(k); dts.append(time.perf_counter() - t0)
        out["host_masking_us_per_frame"] = round(1e6 * statistics.median(dts), 1)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_masks.md"))
    ap.add_argument("--resources", default="", help="the compiler's resource report of the kernel, for the report")
    ap.add_argument("--bench-spread", default="", help="bench.py's own run-to-run spread, quoted beside a difference that lies outside the repeats' spread")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="new", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, ROOT)
        import lvt_amd as lvt
        what, _, kind = a.child.partition(":")
        r = leg_klaunch(lvt, kind) if what == "klaunch" else leg_rgbd(lvt, a.role) if what == "rgbd" else leg_plain(lvt)
        print(json.dumps(r), flush=True)
        return
    me = os.path.abspath(__file__)
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    plain, rgbd = {"new": [], "parent": []}, {"new": [], "parent": []}
    kinds = ("kitti", "tum", "batch16")
    kl = {k: [] for k in kinds}
    for rep in range(a.repeats):   # the two libraries alternate
        if parent:
            plain["parent"].append(run_child([me, "--child", "plain"], lib=parent))
        plain["new"].append(run_child([me, "--child", "plain"]))
        rgbd["parent"].append(run_child([me, "--child", "rgbd", "--role", "parent"], lib=parent))
        rgbd["new"].append(run_child([me, "--child", "rgbd", "--role", "new"]))
        for k in kinds:
            kl[k].append(run_child([me, "--child", "klaunch:" + k]))

    who = "the parent commit's library" if parent else "this commit's library: the parent commit itself was not measured"
    L = ["# Feature masks: key points on masked pixels dropped inside the feature stage", "",
         "Written by `tools/feature_masks.py`.  Synthetic worlds (seed 0) of KITTI (1241 x 376 stereo) and TUM (640 x 480 RGB-D, 16-bit depth) shape; the mask is",
         f"the bonnet (rows below 0.7 H zero).  `sync p50`: host clock around the synchronising call, median of {TIMED} calls.  `async`: frames over wall time,",
         f"{TIMED} frames, three in flight.  Every figure: median of {a.repeats} alternated repeats in child processes of their own (min .. max).", "",
         "## No cost to handles that never set a mask", ""]
    for key, what, lower in (("stereo_async_fps", "stereo headline route, `lvt_amd_track_async`, KITTI-shaped page-locked frames, three in flight [frames/s]", False),
                             ("stereo_sync_p50_us", "`lvt_track`, KITTI-shaped, synchronous p50 [us]", True),
                             ("rgbd_async_fps", "TUM-shaped RGB-D, `lvt_amd_track_rgbd16_async`, pageable frames, three in flight [frames/s]", False)):
        nv, pv = [r[key] for r in plain["new"]], [r[key] for r in plain["parent"]]
        line = f"- {what}: this commit {fmt(nv, 1)}, spread {max(nv) - min(nv):.1f}"
        if pv:
            inside = abs(statistics.median(nv) - statistics.median(pv)) <= max(max(pv) - min(pv), max(nv) - min(nv))
            faster = (statistics.median(nv) < statistics.median(pv)) == lower
            line += f"; parent commit {fmt(pv, 1)}, spread {max(pv) - min(pv):.1f}: the difference of the medians is {'inside' if inside else 'OUTSIDE'} the spread of the repeats" + \
                    ("" if inside else f" (this commit is the {'faster' if faster else 'SLOWER'} one" + (f"; bench.py's own run-to-run spread: {a.bench_spread}" if a.bench_spread else "") + ")")
        else:
            line += "; parent commit: not measured"
        L.append(line)
    bad = sum(r["frames_not_tracking"] for r in plain["new"] + plain["parent"])
    L += ([f"- frames not tracking: {bad}"] if bad else []) + ["", "## The launch", "",
          "`k_mask_features` between its HIP events, as `lvt_amd_profile_read` reports it (the figure includes the event pair's own few microseconds), mean over 100",
          "collected frames per repeat.  One workgroup of 1024 threads per (sequence, eye).", "",
          "| handle | k_mask_features [us] | kept / dropped, left eye of the last frame |", "|---|---|---|"]
    names = {"kitti": "KITTI-shaped pair, both eyes masked", "tum": "TUM-shaped RGB-D image", "batch16": "lock-step batch of 16 KITTI-shaped pairs, every sequence masked"}
    for k in kinds:
        r = kl[k][-1]
        L.append(f"| {names[k]} | {fmt([x['k_mask_features_us'] for x in kl[k]], 2)} | {r['kept'][0]} / {r['dropped'][0]} |")
    L += ["", f"- compiler's resource report: {a.resources or 'see DESIGN.md'}", "", "## RGB-D: the mask inside the tracker against the caller zeroing depth", "",
          "`new`: a masked handle, fed the 16-bit depth plane as the sensor delivers it.  `caller masks`: the only route the parent has, on " + who + " -- the caller",
          "converts the plane to fp32 metres and zeroes it under the mask (numpy, one host core), then calls the fp32 entry.  Stereo has no such route on the parent",
          "commit (the caller would have to run its own detector and hand in external corners), so no stereo comparison is made.", "",
          "| row | new | caller masks | new at least as fast |", "|---|---|---|---|"]
    for key, title, lower in (("sync_p50_us", "synchronous p50 [us]", True), ("async_fps", "host frames, three in flight [frames/s]", False)):
        nv, pv = [r[key] for r in rgbd["new"]], [r[key] for r in rgbd["parent"]]
        ok = statistics.median(nv) <= statistics.median(pv) if lower else statistics.median(nv) >= statistics.median(pv)
        L.append(f"| {title} | {fmt(nv, 1)} | {fmt(pv, 1)} | {'yes' if ok else 'NO'} |")
    bad = sum(r["frames_not_tracking"] for r in rgbd["new"] + rgbd["parent"])
    same = {r["n_left"] for r in rgbd["new"]} == {r["n_left"] for r in rgbd["parent"]}
    L += ["", f"- the caller's conversion and masking of one 640 x 480 plane on one core: {fmt([r['host_masking_us_per_frame'] for r in rgbd['parent']], 1)} us.",
          f"- both routes end their last frame with {'the same' if same else 'DIFFERENT'} feature count; frames not tracking: {bad}."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
