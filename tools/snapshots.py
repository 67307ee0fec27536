#!/usr/bin/env python3
"""Snapshots (lvt_amd_snapshot_*): what taking, applying, exporting and importing a sequence's state costs, and that handles which never snapshot pay
nothing.  Writes profiles/snapshots.md.

  calls     wall time of take / apply / export / import (host clock around the call, median of 30) for
              kitti:    a KITTI-shaped state (1241 x 376, seed 0, 10 frames tracked: about 900 points),
              capacity: a map near its capacity -- the `direct` recipe of tests/case_tables.py (untracked_threshold 1000, nothing is ever culled), 9 frames;
            and the time of the k_state_pack / k_state_unpack launches between HIP events, as lvt_amd_profile_read reports it.
  batch     lvt_amd_batch_snapshot_take on a lock-step batch of 16 KITTI-shaped sequences after 10 steps: one drain, one launch, one read-back.
  plain     a handle that never takes or applies a snapshot, both libraries: the headline route (lvt_amd_track_async, host frames, three in flight) and
            the p50 of the synchronous lvt_track.  The feature must cost it nothing.

--parent-lib names the PARENT commit's liblvt_c.so, built in a worktree of its own; its legs run in child processes of their own (LVT_AMD_LIB) that
alternate with this library's, three times; every figure of `plain` is the median of the three (min .. max).  No threshold is set for the snapshot calls:
the parent commit has nothing to compare them with.  Every child runs under its own time limit; a failing child ends the run (nothing more is started on
the GPU).

  python tools/snapshots.py --parent-lib /path/to/parent/liblvt_c.so [--out profiles/snapshots.md]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NREND, WARM, DEPTH, TIMED, REPS = 40, 20, 3, 300, 30


def pingpong(k):
    p = 2 * (NREND - 1)
    k %= p
    return k if k < NREND else p - k


def clock(fn, n=REPS):
    dts, out = [], None
    for _ in range(n):
        t0 = time.perf_counter(); out = fn(); dts.append(time.perf_counter() - t0)
    return round(1e6 * statistics.median(dts), 1), out


def snapshot_calls(lvt, h, make_target):
    """the four calls on handle h's present state; make_target(): a fresh handle with h's parameters"""
    us_take, snap = clock(h.snapshot)
    info = snap.info
    us_export, raw = clock(snap.to_bytes)
    us_import, imported = clock(lambda: lvt.Snapshot.from_bytes(raw))
    B = make_target()
    us_apply, rc = clock(lambda: B.restore(snap))
    assert rc == 0 and imported.to_bytes() == raw and B.snapshot().to_bytes() == raw, B.last_error()
    for x in (h, B):
        x.profile_enable(True)
    for _ in range(REPS):
        h.snapshot().close()
        assert B.restore(snap) == 0
    prof = {n: (ms, calls) for x in (h, B) for n, ms, calls in x.profile_read() if n.startswith("k_state") and calls}
    B.close()
    return dict(map_n=info["map_n"], staged_n=info["staged_n"], bytes=info["bytes"], take_us=us_take, apply_us=us_apply, export_us=us_export, import_us=us_import,
                pack_launch_us=round(1e3 * prof["k_state_pack"][0] / prof["k_state_pack"][1], 2),
                unpack_launch_us=round(1e3 * prof["k_state_unpack"][0] / prof["k_state_unpack"][1], 2), error=h.last_error())


def kitti_world(lvt):
    from lvt_amd.synth import make_world
    w = make_world("kitti", seed=0)
    return w, lvt.kitti_params(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy, baseline=w.baseline)


def leg(name, lvt):
    import torch
    if name == "calls":
        w, prm = kitti_world(lvt)
        h = lvt.LvtSystem.create(prm, 1)
        for i in range(10):
            h.track(*w.render_stereo(i))
        out = {"kitti": snapshot_calls(lvt, h, lambda: lvt.LvtSystem.create(prm, 1))}
        h.close()
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from case_tables import mapcap_case, mapcap_track
        cprm, frames = mapcap_case("direct", 9)
        h = lvt.LvtSystem.create(cprm, 1)
        for f in frames:
            mapcap_track(h, f)
        out["capacity"] = snapshot_calls(lvt, h, lambda: lvt.LvtSystem.create(cprm, 1))
        h.close()
        return out
    if name == "batch":
        w, prm = kitti_world(lvt)
        pitch = (w.W + 63) // 64 * 64
        dev = torch.zeros((10, 2, w.H, pitch), dtype=torch.uint8, device="cuda")
        for i in range(10):
            a, b = w.render_stereo_torch(i, device="cuda")
            dev[i, 0, :, :w.W], dev[i, 1, :, :w.W] = a, b
        torch.cuda.synchronize()
        batch = lvt.LvtBatch(prm, 16)
        for i in range(10):
            batch.track_device_async([dev[i, 0].data_ptr()] * 16, [dev[i, 1].data_ptr()] * 16, w.H, w.W, pitch)
            batch.wait()

        def take_all():
            for s in batch.snapshot():
                s.close()
        us, _ = clock(take_all)
        snaps = batch.snapshot()
        total = sum(s.info["bytes"] for s in snaps)
        us_apply, rc = clock(lambda: batch.restore_all(snaps))
        assert rc == 0, batch.last_error()
        return dict(batch_take_us=us, batch_apply_us=us_apply, sequences=16, bytes=total, map_n=snaps[0].info["map_n"], error=batch.last_error())
    assert name == "plain"
    w, prm = kitti_world(lvt)
    keep = [w.render_stereo_torch(i, device="cuda").cpu().pin_memory() for i in range(NREND)]
    host = [(t[0].numpy(), t[1].numpy()) for t in keep]
    h = lvt.LvtSystem.create(prm, 1)
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
    out = dict(stereo_async_fps=fps, sync_p50_us=round(1e6 * statistics.median(dts), 1), frames_not_tracking=lost, error=h.last_error())
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


def fmt(v, digits=0):
    return f"{statistics.median(v):.{digits}f} ({min(v):.{digits}f} .. {max(v):.{digits}f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="liblvt_c.so of the parent commit, built in a worktree of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshots.md"))
    ap.add_argument("--resources", default="", help="one line for the report: the state kernels' registers from the compiler's resource report")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, ROOT)
        import lvt_amd as lvt
        print(json.dumps({n: leg(n, lvt) for n in a.child.split(",")}), flush=True)
        return
    me = os.path.abspath(__file__)
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    snap = run_child([me, "--child", "calls,batch"], limit=420)
    plain = {"new": [], "parent": []}
    for _ in range(3):   # the two libraries alternate, three times
        if parent:
            plain["parent"].append(run_child([me, "--child", "plain"], lib=parent, limit=300)["plain"])
        plain["new"].append(run_child([me, "--child", "plain"], limit=300)["plain"])

    L = ["# Snapshots: a sequence's state saved, restored and moved", "",
         "Written by `tools/snapshots.py`.  `take` / `apply` / `export` / `import`: host clock around the call (`LvtSystem.snapshot`, `restore`, `Snapshot.to_bytes`,",
         f"`from_bytes`), median of {REPS} calls on an idle handle; `take` allocates the blob, drains, launches `k_state_pack`, synchronises and reads 16 bytes back; `apply`",
         "launches `k_state_unpack` and synchronises; `export` / `import` move the whole blob over PCIe (pageable host memory) and checksum it on one host core.",
         "`launch`: the time between HIP events around the launch (`lvt_amd_profile_read`; the figure includes the event pair's own few microseconds).",
         "No threshold is set for these: the parent commit has no such calls.", "",
         "| state | map / staged points | bytes | take [us] | apply [us] | export [us] | import [us] | k_state_pack launch [us] | k_state_unpack launch [us] |", "|---|---|---|---|---|---|---|---|---|"]
    for tag, what in (("kitti", "KITTI-shaped, 10 frames"), ("capacity", "`direct` recipe, 9 frames: a map near MAP_MAX")):
        r = snap["calls"][tag]
        L.append(f"| {what} | {r['map_n']} / {r['staged_n']} | {r['bytes']} | {r['take_us']} | {r['apply_us']} | {r['export_us']} | {r['import_us']} | {r['pack_launch_us']} | {r['unpack_launch_us']} |"
                 + (f" error: {r['error']}" if r["error"] else ""))
    b = snap["batch"]
    L += ["", f"- `lvt_amd_batch_snapshot_take` on a lock-step batch of {b['sequences']} KITTI-shaped sequences ({b['map_n']} map points each, {b['bytes']} bytes in all): "
              f"{b['batch_take_us']} us for all of them (one drain, one launch, one read-back; {b['sequences']} allocations and header uploads); "
              f"`lvt_amd_batch_snapshot_apply` of the same {b['sequences']}: {b['batch_apply_us']} us.",
          f"- compiler's resource report for the two kernels: {a.resources or 'see DESIGN.md'}", "", "## No cost to handles that never take or apply a snapshot", "",
          "KITTI-shaped page-locked host frames, 300 frames; the two libraries alternated, medians of three repeats (min .. max)."]
    for key, what, digits in (("stereo_async_fps", "headline route, `lvt_amd_track_async`, three in flight [frames/s]", 1), ("sync_p50_us", "synchronous `lvt_track`, p50 [us]", 1)):
        nv, pv = [r[key] for r in plain["new"]], [r[key] for r in plain["parent"]]
        line = f"- {what}: this commit {fmt(nv, digits)}, spread {max(nv) - min(nv):.1f}"
        if pv:
            inside = abs(statistics.median(nv) - statistics.median(pv)) <= max(max(pv) - min(pv), max(nv) - min(nv))
            line += (f"; parent commit {fmt(pv, digits)}, spread {max(pv) - min(pv):.1f}: the difference of the medians is {'inside' if inside else 'OUTSIDE'} the spread of the repeats")
        else:
            line += "; parent commit: not measured"
        L.append(line)
    bad = sum(r["frames_not_tracking"] for r in plain["new"] + plain["parent"])
    if bad:
        L.append(f"- frames not tracking: {bad}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
