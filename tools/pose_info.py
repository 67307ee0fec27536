#!/usr/bin/env python3
"""Pose uncertainty (lvt_amd_enable_pose_info / k_pose_info): what it costs a handle that enables it, and that a handle which never does pays nothing.
Writes profiles/pose_covariance.md.

  plain     a handle that never enables, both libraries: the headline route (lvt_amd_track_async, page-locked host frames, three in flight) and the p50
            of the synchronous lvt_track.
  enabled   the same two figures on this library with pose info enabled (the synchronous figure: lvt_track alone, and lvt_track followed by
            lvt_amd_get_pose_info, which waits for the frame's tail).
  kernel    k_pose_info between its HIP events (lvt_amd_profile_read; the figure includes the event pair's own few microseconds) on a KITTI-shaped
            frame of a solo handle and on a lock-step batch of 16; and the record's figures for those frames.

--parent-lib names the PARENT commit's liblvt_c.so, built in a worktree of its own; the legs run in child processes of their own (LVT_AMD_LIB) that
alternate -- parent, this library, this library enabled -- three times; every figure is the median of the three (min .. max).  None of these is a
pass / fail number.  Every child runs under its own time limit; a failing child ends the run (nothing more is started on the GPU).

  python tools/pose_info.py --parent-lib /path/to/parent/liblvt_c.so [--out profiles/pose_covariance.md] [--accuracy "..."] [--resources "..."]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NREND, WARM, DEPTH, TIMED = 40, 20, 3, 300


def pingpong(k):
    p = 2 * (NREND - 1)
    k %= p
    return k if k < NREND else p - k


def kitti_world(lvt):
    from lvt_amd.synth import make_world
    w = make_world("kitti", seed=0)
    return w, lvt.kitti_params(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy, baseline=w.baseline)


def leg(name, lvt):
    import numpy as np
    import torch
    w, prm = kitti_world(lvt)
    if name == "kernel":
        h = lvt.LvtSystem.create(prm, 1)
        assert h.enable_pose_info(True) == 0, h.last_error()
        frames = [w.render_stereo(i) for i in range(12)]
        for f in frames[:2]:
            h.track(*f)
        h.profile_enable(True)
        recs = []
        for f in frames[2:]:
            h.track(*f)
            recs.append(h.pose_info())
        prof = {n: (ms, calls) for n, ms, calls in h.profile_read()}
        ms, calls = prof["k_pose_info"]
        pnp_ms, pnp_calls = prof["k_pnp(+project staged)"]
        out = dict(solo_us=round(1e3 * ms / calls, 2), solo_pnp_us=round(1e3 * pnp_ms / pnp_calls, 2), launches=calls,
                   edges=[r.n_edges for r in recs], inliers=[r.n_inliers for r in recs],
                   sigma_p_mm=[round(1e3 * float(np.sqrt(np.diag(r.cov)[:3].max())), 4) for r in recs],
                   sigma_r_mrad=[round(1e3 * float(np.sqrt(np.diag(r.cov)[3:].max())), 4) for r in recs],
                   cond=[round(float(np.linalg.cond(r.info)), 1) for r in recs], error=h.last_error())
        h.close()
        pitch = (w.W + 63) // 64 * 64
        dev = torch.zeros((12, 2, w.H, pitch), dtype=torch.uint8, device="cuda")
        for i in range(12):
            a, b = w.render_stereo_torch(i, device="cuda")
            dev[i, 0, :, :w.W], dev[i, 1, :, :w.W] = a, b
        torch.cuda.synchronize()
        batch = lvt.LvtBatch(prm, 16)
        assert batch.enable_pose_info(True) == 0, batch.last_error()
        for i in range(12):
            if i == 2:
                batch.profile_enable(True)
            batch.track_device_async([dev[i, 0].data_ptr()] * 16, [dev[i, 1].data_ptr()] * 16, w.H, w.W, pitch)
            batch.wait()
        prof = {n: (ms, calls) for n, ms, calls in batch.profile_read()}
        ms, calls = prof["k_pose_info"]
        pnp_ms, pnp_calls = prof["k_pnp(+project staged)"]
        out.update(batch16_us=round(1e3 * ms / calls, 2), batch16_pnp_us=round(1e3 * pnp_ms / pnp_calls, 2),
                   batch_statuses=sorted({batch.pose_info(s).status for s in range(16)}), batch_error=batch.last_error())
        batch.close()
        return out
    enabled = name == "enabled"
    assert name in ("plain", "enabled")
    keep = [w.render_stereo_torch(i, device="cuda").cpu().pin_memory() for i in range(NREND)]
    host = [(t[0].numpy(), t[1].numpy()) for t in keep]
    h = lvt.LvtSystem.create(prm, 1)
    if enabled:
        assert h.enable_pose_info(True) == 0, h.last_error()
    k = 0
    for _ in range(WARM):
        h.track_async(*host[pingpong(k)]); h.wait(); k += 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    inflight, lost = 0, 0
    for _ in range(TIMED):
        h.track_async(*host[pingpong(k)]); k += 1; inflight += 1
        if inflight >= DEPTH:
            lost += int(h.wait_status()[2] != 2); inflight -= 1
    while inflight:
        lost += int(h.wait_status()[2] != 2); inflight -= 1
    fps = round(TIMED / (time.perf_counter() - t0), 1)
    dts = []
    for _ in range(TIMED):
        t0 = time.perf_counter(); h.track(*host[pingpong(k)]); dts.append(time.perf_counter() - t0); k += 1
    lost += int(h.get_state() != 2)
    out = dict(stereo_async_fps=fps, sync_p50_us=round(1e6 * statistics.median(dts), 1), frames_not_tracking=lost)
    if enabled:
        dts, valid = [], 0
        for _ in range(TIMED):
            t0 = time.perf_counter(); h.track(*host[pingpong(k)]); rec = h.pose_info(); dts.append(time.perf_counter() - t0); k += 1
            valid += int(rec.status == 1)
        out.update(sync_with_record_p50_us=round(1e6 * statistics.median(dts), 1), valid_records=valid)
    out["error"] = h.last_error()
    h.close()
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


def fmt(v, digits=1):
    return f"{statistics.median(v):.{digits}f} ({min(v):.{digits}f} .. {max(v):.{digits}f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="liblvt_c.so of the parent commit, built in a worktree of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_covariance.md"))
    ap.add_argument("--resources", default="", help="one line for the report: k_pose_info's registers from the compiler's resource report")
    ap.add_argument("--accuracy", default="", help="one line for the report: the maxima the GPU tests observed against the reference")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, ROOT)
        import lvt_amd as lvt
        print(json.dumps({n: leg(n, lvt) for n in a.child.split(",")}), flush=True)
        return
    me = os.path.abspath(__file__)
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    kern = run_child([me, "--child", "kernel"], limit=300)["kernel"]
    runs = {"parent": [], "plain": [], "enabled": []}
    for _ in range(3):   # the three alternate, three times
        if parent:
            runs["parent"].append(run_child([me, "--child", "plain"], lib=parent, limit=300)["plain"])
        runs["plain"].append(run_child([me, "--child", "plain"], limit=300)["plain"])
        runs["enabled"].append(run_child([me, "--child", "enabled"], limit=300)["enabled"])

    def spread(v):
        return max(v) - min(v)

    L = ["# Pose uncertainty: a per-frame 6x6 covariance from the solver's edges", "",
         "Written by `tools/pose_info.py`.  KITTI-shaped synthetic sequence (1241 x 376, seed 0), page-locked host frames, 300 frames per figure; the legs ran in",
         "child processes that alternated (parent commit's library, this commit never enabled, this commit enabled), medians of three repeats (min .. max).",
         "None of these is a pass / fail number of the test suite.", "",
         "## A handle that never enables it", ""]
    for key, what in (("stereo_async_fps", "headline route, `lvt_amd_track_async`, three in flight [frames/s]"), ("sync_p50_us", "synchronous `lvt_track`, p50 [us]")):
        nv, pv = [r[key] for r in runs["plain"]], [r[key] for r in runs["parent"]]
        line = f"- {what}: this commit {fmt(nv)}, spread {spread(nv):.1f}"
        if pv:
            inside = abs(statistics.median(nv) - statistics.median(pv)) <= max(spread(pv), spread(nv))
            line += f"; parent commit {fmt(pv)}, spread {spread(pv):.1f}: the difference of the medians is {'inside' if inside else 'OUTSIDE'} the spread of the repeats"
        else:
            line += "; parent commit: not measured"
        L.append(line)
    L += ["", "## Enabled", ""]
    for key, what in (("stereo_async_fps", "headline route [frames/s]"), ("sync_p50_us", "synchronous `lvt_track`, p50 [us]"),
                      ("sync_with_record_p50_us", "synchronous `lvt_track` + `lvt_amd_get_pose_info` (waits for the frame's tail), p50 [us]")):
        ev = [r[key] for r in runs["enabled"]]
        line = f"- {what}: {fmt(ev)}, spread {spread(ev):.1f}"
        if key in runs["plain"][0]:
            nv = [r[key] for r in runs["plain"]]
            d = statistics.median(ev) - statistics.median(nv)
            line += f"; never enabled {fmt(nv)}: difference of the medians {d:+.1f} ({100 * d / statistics.median(nv):+.2f} %)"
        L.append(line)
    L.append(f"- valid records among the {TIMED} frames read: {[r['valid_records'] for r in runs['enabled']]}")
    L += ["", "## The kernel", "",
          f"- `k_pose_info` between its HIP events, solo handle, {kern['launches']} KITTI-shaped frames ({min(kern['edges'])} .. {max(kern['edges'])} edges): "
          f"{kern['solo_us']} us per launch (`k_pnp` of the same frames: {kern['solo_pnp_us']} us).",
          f"- lock-step batch of 16 such sequences (gridDim.z = 16): {kern['batch16_us']} us per launch (`k_pnp`: {kern['batch16_pnp_us']} us); record statuses {kern['batch_statuses']}.",
          f"- those frames' records: inliers {min(kern['inliers'])} .. {max(kern['inliers'])}, cond(info) {min(kern['cond'])} .. {max(kern['cond'])}, largest position sigma "
          f"{min(kern['sigma_p_mm'])} .. {max(kern['sigma_p_mm'])} mm, largest rotation sigma {min(kern['sigma_r_mrad'])} .. {max(kern['sigma_r_mrad'])} mrad (unit pixel noise).",
          f"- compiler's resource report: {a.resources or 'see DESIGN.md section 3'}",
          f"- observed against the numpy reference (tests/test_gpu_pose_info.py; bounds 1e-10 / 1e-9 / 1e-9): {a.accuracy or 'see the test output'}"]
    bad = sum(r["frames_not_tracking"] for v in runs.values() for r in v)
    errs = sorted({r["error"] for v in runs.values() for r in v if r["error"]} | {e for e in (kern["error"], kern["batch_error"]) if e})
    if bad:
        L.append(f"- frames not tracking: {bad}")
    if errs:
        L.append(f"- error strings: {errs}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
