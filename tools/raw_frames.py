#!/usr/bin/env python3
"""Raw EuRoC-shaped stereo frames (752 x 480, the reference's cam0 / cam1 calibrations): rectification inside the feature stage (lvt_amd_set_rectifiers)
against the route the PARENT commit offered, the rectifier as a side tool in front of the tracker.  Writes profiles/raw_frames.md.

  sync        one handle, synchronous p50 (host clock around the call, 300 calls), pageable and page-locked buffers.
              new: lvt_track on raw frames.  parent: 2 x lvt_amd_rectify + lvt_track.
  async_dev   one handle, frames/s, raw planes in HBM, three in flight.
              new: raw lvt_amd_track_device_async.  parent: 2 x lvt_amd_rectify_device on a caller stream + event + lvt_amd_track_device_async
              (this leg's handle keeps its private streams, ordered behind nothing of the caller's: the caller waits for the event on the host;
              lvt_amd_set_stream would order the handle behind the caller's stream instead, at the price of the feature stage's overlap).
  async_host  one handle, frames/s, host frames, three in flight.
              new: raw lvt_amd_track_async.  parent: 2 x lvt_amd_rectify to host, then lvt_amd_track_async.
  batch16     a lock-step batch of 16, aggregate frames/s, three steps in flight.
              new: raw lvt_amd_batch_track_device_async.  parent: 32 lvt_amd_rectify_device launches per step in front of the same call.
  plain       a handle WITHOUT rectifiers on rectified frames (lvt_amd_track_device_async, three in flight), both libraries: the feature must cost
              plain handles nothing; and the headline of `python bench.py --gpus 1` under both libraries.

--parent-lib names the PARENT commit's liblvt_c.so, built in a worktree of its own; its legs run in child processes of their own (LVT_AMD_LIB) that
alternate with this library's, three times; every figure is the median of the three (min .. max).  Every leg is a child process under its own time
limit, warm-up first, profiler off, 300 timed frames; a failing leg ends the run (nothing more is started on the GPU).  Frames are rendered once per
child and played forwards and backwards.

  python tools/raw_frames.py --parent-lib /path/to/parent/liblvt_c.so [--out profiles/raw_frames.md] [--no-bench]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NREND, WARM, DEPTH, TIMED, BATCH = 40, 20, 3, 300, 16
W, H, PITCH = 752, 480, 768
P_NEW = [435.2046959714599, 0, 367.4517211914062, 0, 435.2046959714599, 252.2008514404297, 0, 0, 1]
CAMS = [dict(K=[458.654, 0.0, 367.215, 0.0, 457.296, 248.375, 0.0, 0.0, 1.0], D=[-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0],
             R=[0.999966347530033, -0.001422739138722922, 0.008079580483432283, 0.001365741834644127, 0.9999741760894847, 0.007055629199258132,
                -0.008089410156878961, -0.007044357138835809, 0.9999424675829176]),
        dict(K=[457.587, 0.0, 379.999, 0.0, 456.134, 255.238, 0.0, 0.0, 1.0], D=[-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0],
             R=[0.9999633526194376, -0.003625811871560086, 0.007755443660172947, 0.003680398547259526, 0.9999684752771629, -0.007035845251224894,
                -0.007729688520722713, 0.007064130529506649, 0.999945173484644])]


def pingpong(k):
    p = 2 * (NREND - 1)
    k %= p
    return k if k < NREND else p - k


def setup(lvt, seed=1):
    """raw frames of one synthetic EuRoC world in HBM (pitched) and the parameters of the reference's example"""
    import torch
    from lvt_amd.synth import make_world
    w = make_world("euroc", seed=seed)
    assert (w.W, w.H) == (W, H)
    prm = lvt.euroc_params()
    prm.fx = prm.fy = P_NEW[0]
    prm.cx, prm.cy, prm.baseline = P_NEW[2], P_NEW[5], 0.110077842
    prm.img_width, prm.img_height = W, H
    raw = torch.zeros((NREND, 2, H, PITCH), dtype=torch.uint8, device="cuda")
    for i in range(NREND):
        a, b = w.render_stereo_torch(i, device="cuda")
        raw[i, 0, :, :W] = a; raw[i, 1, :, :W] = b
    torch.cuda.synchronize()
    return prm, raw


def rectifiers(lvt):
    return [lvt.Rectifier(c["K"], c["D"], c["R"], P_NEW, W, H) for c in CAMS]


def timed_async(enq, wait, n, per_step=1):
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
    return round(per_step * n / (time.perf_counter() - t0), 1), lost


def leg(name, attached, lvt, prm, raw, rl, rr):
    """attached: this library's route (rectifiers attached, raw frames in); otherwise the parent's route (the rectifier in front of the tracker)"""
    import ctypes as C
    import numpy as np
    import torch
    L = lvt.load_library()
    out = {}

    def rect_dev(src, dst, stream):
        assert L.lvt_amd_rectify_device(rl._h, C.c_void_p(src[0].data_ptr()), PITCH, C.c_void_p(dst[0].data_ptr()), PITCH, C.c_void_p(stream)) == 0
        assert L.lvt_amd_rectify_device(rr._h, C.c_void_p(src[1].data_ptr()), PITCH, C.c_void_p(dst[1].data_ptr()), PITCH, C.c_void_p(stream)) == 0

    def one_wait(h):
        return lambda: int(h.wait_status()[2] != 2)

    if name == "plain":   # rectified planes, made once; a handle without rectifiers
        rect = torch.zeros_like(raw)
        for i in range(NREND):
            rect_dev(raw[i], rect[i], 0)
        torch.cuda.synchronize()
        h = lvt.LvtSystem.create(prm, 1)
        fps, lost = timed_async(lambda k: h.track_device_async(rect[pingpong(k), 0].data_ptr(), rect[pingpong(k), 1].data_ptr(), H, W, PITCH), one_wait(h), TIMED)
        err = h.last_error()
        h.close()
        return dict(plain_async_fps=fps, frames_not_tracking=lost, error=err)

    if name == "sync" or name == "async_host":
        for pin in (False, True):
            mk = (lambda t: t.cpu().pin_memory()) if pin else (lambda t: t.cpu())
            keep = [(mk(raw[i, 0, :, :W].contiguous()), mk(raw[i, 1, :, :W].contiguous())) for i in range(NREND)]
            host = [(a.numpy(), b.numpy()) for a, b in keep]
            ring = [(np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)) for _ in range(DEPTH + 2)]   # the parent's route: rectified host frames, alive while in flight
            h = lvt.LvtSystem.create(prm, 1)
            if attached:
                assert h.set_rectifiers(rl, rr) == 0, h.last_error()
            tag = "pinned" if pin else "pageable"

            def rect_host(k):
                a, b = host[pingpong(k)]
                ra, rb = ring[k % len(ring)]
                assert L.lvt_amd_rectify(rl._h, lvt._p(a), lvt._p(ra)) == 0 and L.lvt_amd_rectify(rr._h, lvt._p(b), lvt._p(rb)) == 0
                return ra, rb
            if name == "sync":
                call = (lambda k: h.track(*host[pingpong(k)])) if attached else (lambda k: h.track(*rect_host(k)))
                k = 0
                for _ in range(WARM):
                    call(k); k += 1
                dts = []
                for _ in range(TIMED):
                    t0 = time.perf_counter(); call(k); dts.append(time.perf_counter() - t0); k += 1
                out[tag] = dict(sync_p50_us=round(1e6 * statistics.median(dts), 1), frames_not_tracking=int(h.get_state() != 2), error=h.last_error())
            else:
                def enq(k):
                    a, b = host[pingpong(k)] if attached else rect_host(k)
                    assert h.track_async(a, b) == 0, h.last_error()
                fps, lost = timed_async(enq, one_wait(h), TIMED)
                out[tag] = dict(async_fps=fps, frames_not_tracking=lost, error=h.last_error())
            h.close()
        return out

    stream = torch.cuda.Stream()
    ev = torch.cuda.Event()
    if name == "async_dev":
        h = lvt.LvtSystem.create(prm, 1)
        ring = torch.zeros((DEPTH + 2, 2, H, PITCH), dtype=torch.uint8, device="cuda")
        if attached:
            assert h.set_rectifiers(rl, rr) == 0, h.last_error()

            def enq(k):
                i = pingpong(k)
                h.track_device_async(raw[i, 0].data_ptr(), raw[i, 1].data_ptr(), H, W, PITCH)
        else:
            def enq(k):
                dst = ring[k % len(ring)]
                rect_dev(raw[pingpong(k)], dst, stream.cuda_stream)
                ev.record(stream); ev.synchronize()
                h.track_device_async(dst[0].data_ptr(), dst[1].data_ptr(), H, W, PITCH)
        fps, lost = timed_async(enq, one_wait(h), TIMED)
        err = h.last_error()
        h.close()
        return dict(async_fps=fps, frames_not_tracking=lost, error=err)

    assert name == "batch16"
    b = lvt.LvtBatch(prm, BATCH)
    ring = torch.zeros((DEPTH + 2, BATCH, 2, H, PITCH), dtype=torch.uint8, device="cuda")
    off = [3 * s for s in range(BATCH)]   # the sequences: one world, every sequence at another place of it
    if attached:
        for s in range(BATCH):
            assert b.set_rectifiers(s, rl, rr) == 0, b.last_error()

        def enq(k):
            fr = [raw[pingpong(k + off[s])] for s in range(BATCH)]
            b.track_device_async([f[0].data_ptr() for f in fr], [f[1].data_ptr() for f in fr], H, W, PITCH)
    else:
        def enq(k):
            dst = ring[k % len(ring)]
            for s in range(BATCH):
                rect_dev(raw[pingpong(k + off[s])], dst[s], stream.cuda_stream)
            ev.record(stream); ev.synchronize()
            b.track_device_async([dst[s, 0].data_ptr() for s in range(BATCH)], [dst[s, 1].data_ptr() for s in range(BATCH)], H, W, PITCH)
    steps = 100
    fps, lost = timed_async(enq, lambda: int((b.wait()[2] != 2).sum()), steps, per_step=BATCH)
    err = b.last_error()
    b.close()
    return dict(async_fps=fps, frames=BATCH * steps, frames_not_tracking=lost, error=err)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_frames.md"))
    ap.add_argument("--legs", default="sync,async_dev,async_host,batch16,plain")
    ap.add_argument("--no-bench", action="store_true", help="skip the bench.py headline of the plain-handle comparison")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--attached", type=int, default=1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:   # one child runs its legs one after the other on ONE set of frames and rectifiers
        sys.path.insert(0, ROOT)
        import lvt_amd as lvt
        prm, raw = setup(lvt)
        rl, rr = rectifiers(lvt)
        print(json.dumps({n: leg(n, bool(a.attached) and n != "plain", lvt, prm, raw, rl, rr) for n in a.child.split(",")}), flush=True)
        return
    me = os.path.abspath(__file__)
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    legs = a.legs.split(",")
    res = {n: {"new": [], "parent": []} for n in legs + ["bench"]}
    for rep in range(3):   # the two libraries alternate, three times
        # the parent's ROUTE (rectifier in front of the tracker); without --parent-lib it is measured on this library, and named so
        rp = run_child([me, "--child", ",".join(n for n in legs if parent or n != "plain"), "--attached", "0"], lib=parent, limit=420)
        rn = run_child([me, "--child", ",".join(legs), "--attached", "1"], limit=420)
        for n in legs:
            if n in rp:
                res[n]["parent"].append(rp[n])
            res[n]["new"].append(rn[n])
        if not a.no_bench:
            bench = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "300", "--warmup", "20", "--no-cpu"]
            if parent:
                res["bench"]["parent"].append(run_child(bench, lib=parent, limit=420))
            res["bench"]["new"].append(run_child(bench, limit=420))

    who = "parent commit" if parent else "this commit, the parent's route"
    L = ["# Raw stereo frames: rectification inside the feature stage", "",
         "Written by `tools/raw_frames.py`.  One synthetic EuRoC world (752 x 480, seed 1), the reference's cam0 / cam1 calibrations, raw frames.",
         "`sync p50`: host clock around the synchronising call, median of 300 calls.  `async`: frames over wall time, 300 frames (batch: 100 steps of 16), three in flight.",
         "Every figure: median of three alternated repeats (min .. max).  `new`: rectifiers attached, raw frames handed to the tracker.",
         f"`parent route` ({who}): the rectifier as a side tool in front of the tracker." if parent else
         "NO --parent-lib: the parent's ROUTE was run on this commit's library; the parent commit itself was not measured.", "",
         "| row | buffers | new | parent route | new is at least as fast |", "|---|---|---|---|---|"]
    verdicts = []

    def row(title, n, tag, key, lower_is_better, unit):
        if n not in res or not res[n]["new"]:
            return
        pick = (lambda r: r[tag][key]) if tag else (lambda r: r[key])
        nv, pv = [pick(r) for r in res[n]["new"]], [pick(r) for r in res[n]["parent"]]
        bad = sum((r[tag] if tag else r)["frames_not_tracking"] for r in res[n]["new"] + res[n]["parent"])
        ok = statistics.median(nv) <= statistics.median(pv) if lower_is_better else statistics.median(nv) >= statistics.median(pv)
        verdicts.append((title, tag, ok))
        L.append(f"| {title} [{unit}] | {tag or 'HBM'} | {fmt(nv, 1 if lower_is_better else 0)} | {fmt(pv, 1 if lower_is_better else 0)} | {'yes' if ok else 'NO'} |"
                 + (f" frames not tracking: {bad}" if bad else ""))
    for tag in ("pageable", "pinned"):
        row("synchronous p50", "sync", tag, "sync_p50_us", True, "us")
    row("asynchronous, planes in HBM", "async_dev", None, "async_fps", False, "frames/s")
    for tag in ("pageable", "pinned"):
        row("asynchronous, host frames", "async_host", tag, "async_fps", False, "frames/s")
    row("batch of 16, aggregate", "batch16", None, "async_fps", False, "frames/s")
    L += ["", "## No cost to plain handles", ""]
    for n, key, what in (("plain", "plain_async_fps", "a handle without rectifiers, EuRoC-shaped rectified frames in HBM, three in flight [frames/s]"),
                         ("bench", "value", "`python bench.py --gpus 1 --steps 300 --warmup 20 --no-cpu` headline")):
        nv = [r.get(key) for r in res[n]["new"] if r.get(key) is not None]
        pv = [r.get(key) for r in res[n]["parent"] if r.get(key) is not None]
        if not nv:
            continue
        line = f"- {what}: this commit {fmt(nv, 1)}, spread {max(nv) - min(nv):.1f}"
        if pv:
            inside = abs(statistics.median(nv) - statistics.median(pv)) <= max(pv) - min(pv)
            line += f"; parent commit {fmt(pv, 1)}, spread {max(pv) - min(pv):.1f}: the difference of the medians is {'inside' if inside else 'OUTSIDE'} the parent's own spread"
        else:
            line += "; parent commit: not measured"
        L.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
