#!/usr/bin/env python3
"""RGB-D throughput on one GPU, TUM-shaped 640 x 480 synthetic sequences; writes profiles/rgbd_batch.md.

  single   one handle: synchronous p50 (host clock around the synchronising call, 300 calls) and asynchronous frames/s (frames over wall time, three in
           flight) for the fp32 / 16-bit HOST entries on pageable and page-locked buffers and the fp32 / 16-bit DEVICE entries.  --parent-lib names the
           PARENT commit's liblvt_c.so (built beside this one): its fp32 host entries are the baseline, run in child processes of their own (LVT_AMD_LIB)
           that alternate with this library's, three times.
  batch    lock-step batches of 1 / 2 / 4 / 8 / 16 RGB-D sequences, planes in HBM, three steps in flight: aggregate frames/s with fp32 and with 16-bit
           depth, alternated three times inside one child per size.
  mixed    one mixed batch of the four calibrations of tests/test_gpu_rgbd_batch.py (distorted, 3 x 2 cells, 320 x 240, 800 x 600 + radius 45).

Every leg is a child process under its own time limit, warm-up first, profiler off, at least 300 timed frames; a failing leg ends the run (nothing more
is started on the GPU).  Frames are rendered into HBM once per child and played forwards and backwards (a continuous motion of any length).

  python tools/rgbd_batch.py --parent-lib /path/to/parent/liblvt_c.so [--out profiles/rgbd_batch.md]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NREND, WARM, DEPTH, TIMED = 60, 20, 3, 300
FR1 = dict(k1=0.262383, k2=-0.953104, p1=-0.005358, p2=0.002628, k3=1.163314)
MIXED = [(84, FR1, (640, 480)), (85, dict(detection_cell_size=300), (640, 480)), (86, {}, (320, 240)), (87, dict(tracking_radius=45), (800, 600))]


def pingpong(k):
    """frame index of step k: 0 .. NREND-1 .. 0 .. (consecutive frames are always neighbours in time)"""
    p = 2 * (NREND - 1)
    k %= p
    return k if k < NREND else p - k


def make_seq(lvt, seed, over, size):
    """one sequence in HBM: gray (pitched), fp32 depth u * s and 16-bit depth u (tight), s = 1 / 5000"""
    import numpy as np
    import torch
    from lvt_amd.synth import make_world
    w = make_world("tum", seed=seed, size=size)
    prm = lvt.tum_params(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy)
    for k, v in over.items():
        setattr(prm, k, type(getattr(prm, k))(v))
    pitch = ((w.W + 63) // 64) * 64
    gray = torch.zeros((NREND, w.H, pitch), dtype=torch.uint8, device="cuda")
    u16 = torch.zeros((NREND, w.H, w.W), dtype=torch.int16, device="cuda")
    for i in range(NREND):
        g, d = w.render_rgbd_torch(i, device="cuda")
        gray[i, :, :w.W] = g
        u16[i] = torch.clamp(torch.round(d.double() * 5000.0), 0, 32767).to(torch.int16)   # (the worlds stay below 22 500 raw units)
    s = float(np.float32(1) / np.float32(5000))
    f32 = u16.to(torch.float32) * torch.tensor(s, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return dict(prm=prm, W=w.W, H=w.H, pitch=pitch, gray=gray, u16=u16, f32=f32, scale=s)


def leg_single(which):
    """which: list of 'entry:pinned' names to run, in order; returns {name: {sync_p50_us, async_fps}}"""
    import numpy as np
    import torch
    import lvt_amd as lvt
    q = make_seq(lvt, 80, {}, (640, 480))
    W, H = q["W"], q["H"]
    host = {}
    for pinned in (False, True):
        mk = (lambda t: t.cpu().pin_memory()) if pinned else (lambda t: t.cpu())
        keep = [(mk(q["gray"][i, :, :W].contiguous()), mk(q["f32"][i]), mk(q["u16"][i])) for i in range(NREND)]
        host[pinned] = (keep, [(g.numpy(), f.numpy(), u.numpy().view(np.uint16)) for g, f, u in keep])
    out = {}
    for name in which:
        entry, pin = name.split(":")
        arrs = host[pin == "pinned"][1]
        h = lvt.LvtSystem.create(q["prm"], 2)
        if entry == "host_f32":
            sync = lambda i: h.track(arrs[i][0], arrs[i][1])                                     # noqa: E731
            enq = lambda i: h.track_async(arrs[i][0], arrs[i][1])                                # noqa: E731
        elif entry == "host_u16":
            sync = lambda i: h.track(arrs[i][0], arrs[i][2], depth_scale=q["scale"])             # noqa: E731
            enq = lambda i: h.track_async(arrs[i][0], arrs[i][2], depth_scale=q["scale"])        # noqa: E731
        else:
            fmt = lvt.DEPTH_U16 if entry == "dev_u16" else lvt.DEPTH_F32
            pl, dp = (q["u16"], 2 * W) if fmt == lvt.DEPTH_U16 else (q["f32"], 4 * W)
            gp, dpt = [q["gray"][i].data_ptr() for i in range(NREND)], [pl[i].data_ptr() for i in range(NREND)]
            sync = lambda i: h.track_rgbd_device(gp[i], dpt[i], H, W, q["pitch"], dp, fmt, q["scale"])         # noqa: E731
            enq = lambda i: h.track_rgbd_device_async(gp[i], dpt[i], H, W, q["pitch"], dp, fmt, q["scale"])    # noqa: E731
        k = 0
        for _ in range(WARM):
            sync(pingpong(k)); k += 1
        dts = []
        for _ in range(TIMED):
            t0 = time.perf_counter(); sync(pingpong(k)); dts.append(time.perf_counter() - t0); k += 1
        lost = int(h.get_state() != 2)
        for _ in range(WARM):
            assert enq(pingpong(k)) == 0, h.last_error()
            h.wait_status(); k += 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inflight = 0
        for _ in range(TIMED):
            assert enq(pingpong(k)) == 0, h.last_error()
            k += 1; inflight += 1
            if inflight >= DEPTH:
                lost += int(h.wait_status()[2] != 2); inflight -= 1
        while inflight:
            lost += int(h.wait_status()[2] != 2); inflight -= 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[name] = dict(sync_p50_us=round(1e6 * statistics.median(dts), 1), async_fps=round(TIMED / dt, 1), frames_not_tracking=lost, error=h.last_error(),
                         planes_in_place=h.host_stats()["planes_in_place"])
        h.close()
    return out


def leg_batch(cases):
    """cases: [(seed, overrides, size)]: one lock-step batch of them (uniform when all share a parameter set), fp32 and 16-bit alternated three times"""
    import torch
    import lvt_amd as lvt
    seqs = [make_seq(lvt, *c) for c in cases]
    B = len(seqs)
    uniform = len({bytes(q["prm"].to_pod()) for q in seqs}) == 1
    steps = max(100, -(-TIMED // B))
    H, W, GP = [q["H"] for q in seqs], [q["W"] for q in seqs], [q["pitch"] for q in seqs]
    res = {"f32": [], "u16": []}
    for rep in range(3):
        for name in ("f32", "u16"):
            fmt = lvt.DEPTH_U16 if name == "u16" else lvt.DEPTH_F32
            b = lvt.LvtBatch(seqs[0]["prm"], B, sensor_type=2) if uniform else lvt.LvtBatch.create_mixed([q["prm"] for q in seqs], sensor_type=2)
            key, esz = ("u16", 2) if name == "u16" else ("f32", 4)
            DP = [esz * w for w in W]

            def enq(k):
                i = pingpong(k)
                rc = b.track_rgbd_device_async([q["gray"][i].data_ptr() for q in seqs], [q[key][i].data_ptr() for q in seqs], H, W, GP, DP, fmt, seqs[0]["scale"])
                assert rc == 0, b.last_error()
            k = 0
            for _ in range(WARM):
                enq(k); b.wait(); k += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inflight, lost = 0, 0
            for _ in range(steps):
                enq(k); k += 1; inflight += 1
                if inflight >= DEPTH:
                    lost += int((b.wait()[2] != 2).sum()); inflight -= 1
            while inflight:
                lost += int((b.wait()[2] != 2).sum()); inflight -= 1
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[name].append(dict(fps=round(B * steps / dt, 1), frames=B * steps, frames_not_tracking=lost, error=b.last_error()))
            b.close()
    return dict(B=B, uniform=uniform, **res)


def child(a):
    sys.path.insert(0, ROOT)
    if a.leg == "single":
        print(json.dumps(leg_single(a.which.split(","))), flush=True)
    elif a.leg == "batch":
        print(json.dumps(leg_batch([(80 + s, {}, (640, 480)) for s in range(a.B)])), flush=True)
    else:
        print(json.dumps(leg_batch(MIXED)), flush=True)


def run_child(args, lib=None, limit=300):
    env = dict(os.environ)
    if lib:
        env["LVT_AMD_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args, capture_output=True, text=True, timeout=limit, env=env)
    if out.returncode != 0:   # a failed leg ends the run: nothing more is started on the GPU
        print(json.dumps({"leg": args, "failed": out.returncode, "stderr": out.stderr[-3000:]}), flush=True)
        raise SystemExit(1)
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps({"leg": args, "lib": lib or "this checkout", "result": r}), flush=True)
    return r


def med_spread(v):
    return statistics.median(v), max(v) - min(v)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="liblvt_c.so of the parent commit (the baseline of the fp32 host entries)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgbd_batch.md"))
    ap.add_argument("--sizes", default="1,2,4,8,16")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--leg", default="single", help=argparse.SUPPRESS)
    ap.add_argument("--which", default="", help=argparse.SUPPRESS)
    ap.add_argument("--B", type=int, default=1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    host_f32 = ["host_f32:pageable", "host_f32:pinned"]
    new_all = host_f32 + ["host_u16:pageable", "host_u16:pinned", "dev_f32:-", "dev_u16:-"]
    single = {"parent": [], "new": []}
    for rep in range(3):   # parent / this library alternate, three times
        if a.parent_lib:
            single["parent"].append(run_child(["--leg", "single", "--which", ",".join(host_f32)], lib=os.path.abspath(a.parent_lib)))
        single["new"].append(run_child(["--leg", "single", "--which", ",".join(new_all)]))
    batches = [run_child(["--leg", "batch", "--B", str(B)], limit=420) for B in [int(x) for x in a.sizes.split(",")]]
    mixed = run_child(["--leg", "mixed"], limit=420)

    L = ["# RGB-D: device-resident planes, 16-bit depth, lock-step batches", "",
         "Written by `tools/rgbd_batch.py`.  TUM-shaped synthetic sequences (640 x 480, seeds 80 ...), 16-bit depth u = round(5000 d), fp32 depth u / 5000.",
         "`sync p50`: host clock around the synchronising call, median of 300 calls.  `async`: frames over wall time, 300 frames, three in flight.",
         "Every figure: median of three alternated repeats (min .. max).", "", "## One handle", "",
         "| library | entry | buffers | sync p50 [us] | async [frames/s] |", "|---|---|---|---|---|"]
    stats = {}
    for lib in ("parent", "new"):
        if not single[lib]:
            continue
        for name in (host_f32 if lib == "parent" else new_all):
            sp = [r[name]["sync_p50_us"] for r in single[lib]]
            fp = [r[name]["async_fps"] for r in single[lib]]
            bad = sum(r[name]["frames_not_tracking"] for r in single[lib])
            errs = sorted({r[name]["error"] for r in single[lib]} - {""})
            stats[(lib, name)] = (med_spread(sp), med_spread(fp))
            e, p = name.split(":")
            L.append(f"| {'parent commit' if lib == 'parent' else 'this commit'} | {e} | {p} | {statistics.median(sp):.1f} ({min(sp):.1f} .. {max(sp):.1f}) | "
                     f"{statistics.median(fp):.0f} ({min(fp):.0f} .. {max(fp):.0f}) |" + (f" not tracking: {bad}" if bad else "") + (f" errors: {errs}" if errs else ""))
    L += ["", "## Lock-step batches (planes in HBM, three steps in flight)", "", "| sequences | fp32 [frames/s, aggregate] | 16-bit [frames/s, aggregate] |", "|---|---|---|"]
    bstats = {}
    for r in batches + [mixed]:
        cells = []
        for k in ("f32", "u16"):
            v = [x["fps"] for x in r[k]]
            bad = sum(x["frames_not_tracking"] for x in r[k])
            bstats[(r["B"], r["uniform"], k)] = med_spread(v)
            cells.append(f"{statistics.median(v):.0f} ({min(v):.0f} .. {max(v):.0f})" + (f" not tracking: {bad}" if bad else ""))
        L.append(f"| {r['B']}{'' if r['uniform'] else ' (mixed: fr1 distortion, 3 x 2 cells, 320 x 240, 800 x 600 + radius 45)'} | {cells[0]} | {cells[1]} |")
    L += ["", "## Conditions", ""]
    if single["parent"]:
        for p in ("pageable", "pinned"):
            (ps, pss), (pf, pfs) = stats[("parent", f"host_f32:{p}")]
            (ns, _), (nf, _) = stats[("new", f"host_f32:{p}")]
            (us, _), (uf, _) = stats[("new", f"host_u16:{p}")]
            L.append(f"- (a) fp32 host, {p}: sync p50 {ns:.1f} us against the parent's {ps:.1f} (parent's own spread {pss:.1f}): {'holds' if ns <= ps + pss else 'MISSED'}; "
                     f"async {nf:.0f} against {pf:.0f} frames/s (spread {pfs:.0f}): {'holds' if nf >= pf - pfs else 'MISSED'}")
            L.append(f"- (b) 16-bit host against fp32 host of this commit, {p}: sync p50 {us:.1f} against {ns:.1f} us: {'holds' if us <= ns + pss else 'MISSED'}; "
                     f"async {uf:.0f} against {nf:.0f} frames/s: {'holds' if uf >= nf - pfs else 'MISSED'}")
        base, bsp = stats[("parent", "host_f32:pageable")][1]
        basep = stats[("parent", "host_f32:pinned")][1][0]
        for k in ("f32", "u16"):
            if (8, True, k) in bstats:
                v, sp = bstats[(8, True, k)]
                L.append(f"- (c) batch of 8, {k}: {v:.0f} frames/s aggregate (spread {sp:.0f}) against the parent's single asynchronous handle at {base:.0f} (pageable; "
                         f"{basep:.0f} page-locked; spread {bsp:.0f}): {'holds' if v - sp > max(base, basep) + bsp else 'MISSED'}")
    else:
        L.append("(no --parent-lib: the parent baseline was not run)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
