#!/usr/bin/env python3
"""Frames/s of eight KITTI-00..07-shaped synthetic sequences (three image sizes, three calibrations) on one GPU:

  mixed          (a) ONE mixed lock-step batch of the eight (lvt_amd_batch_create_mixed)
  three_uniform  (b) what a build without mixed batches offers them: three uniform batches of 3 / 1 / 4 sequences, driven round-robin from one thread
  solo8          (c) ... or eight solo handles on eight threads
  uniform8       (d) a uniform batch of eight 1241 x 376 sequences (the existing path: must not change)

Frames are rendered into HBM first; 4 warm-up steps, then the timed steps with three in flight, a device synchronisation either side of the
timed part (the discipline of bench.py's batch leg).  Every mode runs in a child process of its own, `--repeats` times; one JSON line per mode.
--package-root DIR measures ANOTHER checkout's lvt_amd package and library (modes b, c, d on the parent commit).

  python tools/mixed_batch.py --mode all --frames 104 --repeats 3
"""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

SHAPES = [(1241, 376)] * 3 + [(1242, 375)] + [(1226, 370)] * 4   # KITTI odometry 00 - 02, 03, 04 - 07
GROUPS = [[0, 1, 2], [3], [4, 5, 6, 7]]
WARM, DEPTH = 4, 3


def make_sequences(lvt, shapes, n):
    import torch
    from lvt_amd.synth import make_world
    seqs = []
    for s, size in enumerate(shapes):
        w = make_world("kitti", seed=100 + s, size=size)
        prm = lvt.kitti_params(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy, baseline=w.baseline)
        pitch = ((w.W + 63) // 64) * 64
        fr = torch.zeros((n, 2, w.H, pitch), dtype=torch.uint8, device="cuda")
        for i in range(n):
            fr[i, :, :, :w.W] = w.render_stereo_torch(i, device="cuda")
        seqs.append(dict(prm=prm, W=w.W, H=w.H, pitch=pitch, fr=fr, l=[fr[i, 0].data_ptr() for i in range(n)], r=[fr[i, 1].data_ptr() for i in range(n)]))
    torch.cuda.synchronize()
    return seqs


def drive(batches, n):
    """batches: list of (enqueue(i), wait() -> states); all of them advance step by step from this thread.  Returns (seconds, frames not TRACKING)"""
    import torch
    for i in range(WARM):
        for enq, wait in batches:
            enq(i); wait()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    inflight, bad = 0, 0
    for i in range(WARM, n):
        for enq, _ in batches:
            enq(i)
        inflight += 1
        if inflight >= DEPTH:
            bad += sum(int((wait() != 2).sum()) for _, wait in batches); inflight -= 1
    while inflight:
        bad += sum(int((wait() != 2).sum()) for _, wait in batches); inflight -= 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0, bad


def run_mode(mode, n):
    import torch
    import lvt_amd as lvt
    errs = []
    if mode == "uniform8":
        seqs = make_sequences(lvt, [SHAPES[0]] * 8, n)
    else:
        seqs = make_sequences(lvt, SHAPES, n)
    if mode == "mixed":
        b = lvt.LvtBatch.create_mixed([q["prm"] for q in seqs])
        H, W, P = [q["H"] for q in seqs], [q["W"] for q in seqs], [q["pitch"] for q in seqs]

        def enq(i):
            assert b.track_device_async_mixed([q["l"][i] for q in seqs], [q["r"][i] for q in seqs], H, W, P) == 0, b.last_error()
        dt, bad = drive([(enq, lambda: b.wait()[2])], n)
        errs.append(b.last_error()); b.close()
    elif mode in ("three_uniform", "uniform8"):
        groups = GROUPS if mode == "three_uniform" else [list(range(8))]
        hs, batches = [], []
        for g in groups:
            q0 = seqs[g[0]]
            b = lvt.LvtBatch(q0["prm"], len(g))
            hs.append(b)
            batches.append((lambda i, b=b, g=g, q0=q0: b.track_device_async([seqs[s]["l"][i] for s in g], [seqs[s]["r"][i] for s in g], q0["H"], q0["W"], q0["pitch"]),
                            lambda b=b: b.wait()[2]))
        dt, bad = drive(batches, n)
        for b in hs:
            errs.append(b.last_error()); b.close()
    elif mode == "solo8":
        hs = [lvt.LvtSystem.create(q["prm"], 1) for q in seqs]
        start, bads = threading.Barrier(len(seqs) + 1), [0] * len(seqs)

        def worker(k):
            h, q = hs[k], seqs[k]
            for i in range(WARM):
                h.track_device_async(q["l"][i], q["r"][i], q["H"], q["W"], q["pitch"]); h.wait_status()
            start.wait()
            inflight = 0
            for i in range(WARM, n):
                h.track_device_async(q["l"][i], q["r"][i], q["H"], q["W"], q["pitch"]); inflight += 1
                if inflight >= DEPTH:
                    bads[k] += int(h.wait_status()[2] != 2); inflight -= 1
            while inflight:
                bads[k] += int(h.wait_status()[2] != 2); inflight -= 1
        th = [threading.Thread(target=worker, args=(k,)) for k in range(len(seqs))]
        for t in th:
            t.start()
        start.wait()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in th:
            t.join()
        torch.cuda.synchronize()
        dt, bad = time.perf_counter() - t0, sum(bads)
        for h in hs:
            errs.append(h.last_error()); h.close()
    else:
        raise SystemExit(f"unknown mode {mode}")
    frames = 8 * (n - WARM)
    return {"mode": mode, "fps": round(frames / dt, 1), "frames": frames, "seconds": round(dt, 4), "frames_not_tracking": bad, "errors": sorted(set(e for e in errs if e))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", default="all", choices=["all", "mixed", "three_uniform", "solo8", "uniform8"])
    ap.add_argument("--frames", type=int, default=104, help="frames per sequence, the first 4 of them warm-up")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--package-root", default=None, help="a checkout whose lvt_amd package and built library are measured instead of this one's")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    root = os.path.abspath(a.package_root or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    if a.child:
        sys.path.insert(0, root)
        print(json.dumps(run_mode(a.mode, a.frames)), flush=True)
        return
    modes = ["mixed", "three_uniform", "solo8", "uniform8"] if a.mode == "all" else [a.mode]
    for m in modes:
        reps = []
        for _ in range(a.repeats):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--mode", m, "--frames", str(a.frames), "--package-root", root]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:   # a failed child ends the run: nothing more is started on the GPU
                print(json.dumps({"mode": m, "failed": out.returncode, "stderr": out.stderr[-2000:]}), flush=True)
                raise SystemExit(1)
            reps.append(json.loads(out.stdout.strip().splitlines()[-1]))
        fps = sorted(r["fps"] for r in reps)
        print(json.dumps({"mode": m, "package_root": root, "fps_median": fps[len(fps) // 2], "fps_min": fps[0], "fps_max": fps[-1], "spread": round(fps[-1] - fps[0], 1),
                          "repeats": reps}), flush=True)


if __name__ == "__main__":
    main()
