#!/usr/bin/env python3
"""Per-frame label masks (lvt_amd_set_label_mask, lvt_amd_frame_labels*): what the launch costs, what the feature buys over the parent commit's only route, and
that it costs a handle that never sets a record nothing.  Writes profiles/label_masks.md.

  plain    handles that never set a record, both libraries: the stereo headline route (lvt_amd_track_async, KITTI-shaped page-locked frames, three in flight),
           the synchronous p50 of lvt_track, the TUM-shaped RGB-D route (lvt_amd_track_rgbd16_async).
  klaunch  k_label_mask between its HIP events (lvt_amd_profile_read), 50 collected frames per row: a KITTI-shaped pair (1241 x 376, both eyes labelled), a
           TUM-shaped image (640 x 480) and a lock-step batch of 16 KITTI-shaped pairs, at dilate 0 / 4 / 15 and label scale 1 and 1/4.
  buys     a new label image (quarter scale, in HBM) for the left eye of every KITTI-shaped frame, dilate 4.  new: lvt_amd_frame_labels_device +
           lvt_amd_track_async, three frames in flight; and the same synchronously for the p50.  parent: the only route the parent commit has -- the caller
           builds the plane with torch on the device (table look-up, nearest upsample by index, max_pool2d), waits for it, collects every frame,
           calls lvt_amd_set_mask_device and tracks.
  The EFFECT row of the issue (the share of map points on a block that moves against the scene) is not produced by this tool: not measured.

--parent-lib names the PARENT commit's liblvt_c.so, built in a worktree of its own; its legs run in child processes of their own (LVT_AMD_LIB) that alternate
with this library's, three times; every figure is the median of the three (min .. max).  Every child runs under its own time limit, warm-up first, profiler
off (but for klaunch); a failing child ends the run (nothing more is started on the GPU).

  python tools/label_masks.py --parent-lib /path/to/parent/liblvt_c.so [--out profiles/label_masks.md] [--resources "..."]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from feature_masks import ROOT, NREND, WARM, TIMED, SCALE, pingpong, timed_async, timed_sync, stereo_world, rgbd_world, leg_plain, run_child, fmt  # noqa: E402

DROPPED, DILATES, BUYS_DILATE = (11, 13), (0, 4, 15), 4


def labels_of(LW, LH, i):
    """label 7 everywhere, a block of 13 sliding right and a block of 11 sliding left (the tests' sequence, on a ping-pong frame number)"""
    import numpy as np
    lab = np.full((LH, LW), 7, np.uint8)
    c0, c1 = int(0.10 * LW) + (6 * i) % max(1, LW // 2), int(0.80 * LW) - (4 * i) % max(1, LW // 2)
    lab[int(0.3 * LH):int(0.9 * LH), c0:c0 + int(0.22 * LW)] = 13
    lab[int(0.4 * LH):int(0.8 * LH), max(0, c1):max(0, c1) + max(1, int(0.06 * LW))] = 11
    return lab


def device_labels(LW, LH):
    import torch
    return torch.stack([torch.from_numpy(labels_of(LW, LH, i)) for i in range(NREND)]).cuda().contiguous()


def leg_klaunch(lvt, kind):
    import torch
    B = 16 if kind == "batch16" else 1
    if kind == "tum":
        w, prm, fr = rgbd_world(lvt)
        h = lvt.LvtSystem.create(prm, 2)
        track = lambda k: h.track(*fr[pingpong(k)], depth_scale=SCALE)   # noqa: E731
    elif kind == "kitti":
        w, prm, keep, host = stereo_world(lvt)
        h = lvt.LvtSystem.create(prm, 1)
        track = lambda k: h.track(*host[pingpong(k)])   # noqa: E731
    else:
        w, prm, keep, host = stereo_world(lvt)
        pitch = (w.W + 63) // 64 * 64
        dev = torch.zeros((NREND, 2, w.H, pitch), dtype=torch.uint8, device="cuda")
        for i, t in enumerate(keep):
            dev[i, :, :, :w.W] = t.cuda()
        torch.cuda.synchronize()
        h = lvt.LvtBatch(prm, B)

        def track(k):
            i = pingpong(k)
            h.track_device_async([dev[i, 0].data_ptr()] * B, [dev[i, 1].data_ptr()] * B, w.H, w.W, pitch)
            h.wait()
    rows = {}
    for scale in (1, 4):
        LW, LH = (w.W + scale - 1) // scale, (w.H + scale - 1) // scale
        labs = device_labels(LW, LH)
        torch.cuda.synchronize()
        for d in DILATES:
            h.profile_enable(False)
            rec = lvt.LabelMask(LW, LH, DROPPED, d)
            for s in range(B):
                assert (h.set_label_mask(s, rec) if B > 1 else h.set_label_mask(rec)) == 0, h.last_error()

            def frame(k):
                p = labs[pingpong(k)].data_ptr()
                right = 0 if kind == "tum" else p
                for s in range(B):
                    assert (h.frame_labels(s, p, right, LW, LW) if B > 1 else h.frame_labels(p, right, LW, LW)) == 0, h.last_error()
                track(k)
            for k in range(8):
                frame(k)
            h.profile_enable(True)
            for k in range(50):
                frame(8 + k)
            prof = {n: (ms, calls) for n, ms, calls in h.profile_read()}
            ms, calls = prof["k_label_mask"]
            assert calls == 50, prof
            st = h.mask_stats(0) if B > 1 else h.mask_stats()
            rows[f"1/{scale} d{d}"] = {"us": round(1e3 * ms / calls, 2), "dropped": st["dropped"][0], "kept": st["kept"][0]}
    out = {"rows": rows, "error": h.last_error()}
    h.close()
    return out


def leg_buys(lvt, role):
    import numpy as np
    import torch
    import torch.nn.functional as F
    w, prm, keep, host = stereo_world(lvt)
    LW, LH, r = (w.W + 3) // 4, (w.H + 3) // 4, BUYS_DILATE
    labs = device_labels(LW, LH)
    h = lvt.LvtSystem.create(prm, 1)
    new = role == "new"
    if new:
        assert h.set_label_mask(lvt.LabelMask(LW, LH, DROPPED, r)) == 0, h.last_error()
    table = torch.zeros(256, dtype=torch.bool, device="cuda")
    table[list(DROPPED)] = True
    lx = (torch.arange(w.W, device="cuda") * LW) // w.W
    ly = (torch.arange(w.H, device="cuda") * LH) // w.H
    plane = torch.zeros((w.H, w.W), dtype=torch.uint8, device="cuda")

    def caller_builds(k):
        f0 = table[labs[pingpong(k)].long()][ly][:, lx].float()[None, None]
        f = F.max_pool2d(f0, 2 * r + 1, 1, r)[0, 0]
        plane.copy_(((1.0 - f) * 255).to(torch.uint8))
        torch.cuda.synchronize()   # (the tracker copies the plane on its own stream)
        assert h.set_mask_device(plane.data_ptr(), w.W, 0, 0) == 0, h.last_error()

    def sync(k):
        if new:
            assert h.frame_labels(labs[pingpong(k)].data_ptr(), 0, LW, 0) == 0, h.last_error()
        else:
            caller_builds(k)
        h.track(*host[pingpong(k)])
    out = {"sync_p50_us": timed_sync(sync)}
    bad = int(h.get_state() != 2)
    if new:
        def enq(k):
            assert h.frame_labels(labs[pingpong(k)].data_ptr(), 0, LW, 0) == 0, h.last_error()
            assert h.track_async(*host[pingpong(k)]) == 0, h.last_error()
        out["fps"], lost = timed_async(enq, lambda: int(h.wait_status()[2] != 2), TIMED)
    else:   # a set needs a quiet handle: one frame at a time is all the parent's route allows
        for k in range(WARM):
            sync(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lost = 0
        for k in range(TIMED):
            sync(WARM + k)
            lost += int(h.get_state() != 2)
        out["fps"] = round(TIMED / (time.perf_counter() - t0), 1)
    st = h.mask_stats()
    out.update(frames_not_tracking=bad + lost, error=h.last_error(), dropped=st["dropped"][0], kept=st["kept"][0])
    if new:   # the two routes build the same plane
        caller = ((1.0 - F.max_pool2d(table[labs[0].long()][ly][:, lx].float()[None, None], 2 * r + 1, 1, r)[0, 0]) * 255).to(torch.uint8).cpu().numpy()
        got = lvt.build_label_mask(lvt.LabelMask(LW, LH, DROPPED, r), np.ascontiguousarray(labs[0].cpu().numpy()), w.W, w.H)[:, :w.W]
        out["planes_equal"] = bool(np.array_equal(caller, got))
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="liblvt_c.so of the parent commit, built in a worktree of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_masks.md"))
    ap.add_argument("--resources", default="", help="the compiler's resource report of the kernel, for the report")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="new", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, ROOT)
        import lvt_amd as lvt
        what, _, kind = a.child.partition(":")
        r = leg_klaunch(lvt, kind) if what == "klaunch" else leg_buys(lvt, a.role) if what == "buys" else leg_plain(lvt)
        print(json.dumps(r), flush=True)
        return
    me = os.path.abspath(__file__)
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    plain, buys = {"new": [], "parent": []}, {"new": [], "parent": []}
    kinds = ("kitti", "tum", "batch16")
    kl = {k: [] for k in kinds}
    for rep in range(a.repeats):   # the two libraries alternate
        if parent:
            plain["parent"].append(run_child([me, "--child", "plain"], lib=parent))
        plain["new"].append(run_child([me, "--child", "plain"]))
        buys["parent"].append(run_child([me, "--child", "buys", "--role", "parent"], lib=parent))
        buys["new"].append(run_child([me, "--child", "buys", "--role", "new"]))
        for k in kinds:
            kl[k].append(run_child([me, "--child", "klaunch:" + k]))

    who = "the parent commit's library" if parent else "this commit's library: the parent commit itself was not measured"
    L = ["# Per-frame label masks: a segmentation image travels with each frame", "",
         "Written by `tools/label_masks.py`.  Synthetic worlds (seed 0) of KITTI (1241 x 376 stereo) and TUM (640 x 480 RGB-D, 16-bit depth) shape; the label",
         "images hold two sliding blocks of dropped labels (11 and 13).  `sync p50`: host clock around the synchronising call, median of " + f"{TIMED} calls.",
         f"`async`: frames over wall time, {TIMED} frames, three in flight.  Every figure: median of {a.repeats} alternated repeats in child processes of their own",
         "(min .. max).", "", "## No cost to handles that never set a record", ""]
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
          "`k_label_mask` between its HIP events, as `lvt_amd_profile_read` reports it (the figure includes the event pair's own few microseconds), mean over 50",
          "collected frames per repeat.  A workgroup of 256 threads per 32 x 32 tile of the plane; every labelled eye of the step in one launch.", "",
          "| handle | label scale | dilate 0 [us] | dilate 4 [us] | dilate 15 [us] |", "|---|---|---|---|---|"]
    names = {"kitti": "KITTI-shaped pair, both eyes labelled", "tum": "TUM-shaped RGB-D image", "batch16": "lock-step batch of 16 KITTI-shaped pairs, every eye labelled"}
    for k in kinds:
        for scale in (1, 4):
            cells = [fmt([x["rows"][f"1/{scale} d{d}"]["us"] for x in kl[k]], 2) for d in DILATES]
            L.append(f"| {names[k]} | {'1' if scale == 1 else '1/4'} | " + " | ".join(cells) + " |")
    L += ["", f"- compiler's resource report: {a.resources or 'see DESIGN.md'}", "", "## What the feature buys: a new label image with every frame", "",
          f"KITTI-shaped frames in page-locked host memory, a quarter-scale label image in HBM for the left eye of every frame, dilate {BUYS_DILATE}.  `new`:",
          "`lvt_amd_frame_labels_device` + `lvt_amd_track_async`, three frames in flight (p50: the same through `lvt_track`).  `caller builds`: the only route the",
          "parent has, on " + who + " -- torch on the device (table look-up, nearest upsample by index, `max_pool2d`), a wait for it, every frame collected,",
          "`lvt_amd_set_mask_device`, `lvt_track`.", "", "| row | new | caller builds | new at least as fast |", "|---|---|---|---|"]
    for key, title, lower in (("fps", "frames/s", False), ("sync_p50_us", "p50 of one frame, labels to pose [us]", True)):
        nv, pv = [r[key] for r in buys["new"]], [r[key] for r in buys["parent"]]
        ok = statistics.median(nv) <= statistics.median(pv) if lower else statistics.median(nv) >= statistics.median(pv)
        L.append(f"| {title} | {fmt(nv, 1)} | {fmt(pv, 1)} | {'yes' if ok else 'NO'} |")
    bad = sum(r["frames_not_tracking"] for r in buys["new"] + buys["parent"])
    same = all(r.get("planes_equal") for r in buys["new"])
    L += ["", f"- the caller's torch plane and `k_label_mask`'s plane of the same label image are {'equal byte for byte' if same else 'DIFFERENT'}; frames not tracking: {bad}.",
          "", "## Effect on a block that moves against the scene", "", "Not measured."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
