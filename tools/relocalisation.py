#!/usr/bin/env python3
"""Relocalisation: what the call costs, and what it costs a handle that never makes it (results: profiles/relocalisation.md).

    python tools/relocalisation.py [--parent-lib PATH/liblvt_c.so] [--repeats 3]
    python tools/relocalisation.py --kernel-trace        every launch's own duration: the `call`, `fullmap` and `capacity` legs each once under
                                                         rocprofv3 --kernel-trace --stats (no counters), the rows of the relocalisation kernels

Every leg runs in a child process of its own (one HIP runtime, one library per process); with --parent-lib the legs that have a counterpart in the parent
commit's library (headline route, synchronous lvt_track) alternate parent / this tree, `repeats` times each, and medians are printed with every repeat beside
them.  Legs:
  match      lvt_amd_reloc_match_device at 1 052 x 844 and 4 096 x 32 768, both variants (LDS staging, the one the library ships; LVT_AMD_RELOC_MATCH=uniform),
             time between HIP events around the two launches, median of 20 calls behind 5
  call       lvt_amd_relocalise (dry run) on a full-size synthetic KITTI state -- 8 frames, a flat frame, frame 12 --, host clock around the call
  fullmap    lvt_amd_relocalise (dry run) on a handle whose map is FULL: twelve frames of noise with ~4 000 external corners each and a culling threshold of
             1 000 frames (every frame's fresh corners triangulate, nothing is culled: the map reaches its 32 768 points in the ninth frame and is cut there,
             which the handle reports as a capacity overflow), a flat frame, then the fifth noise frame again (its ~4 000 corners are all in the map); host clock
             around the call
  capacity   the capacity shapes as a COMPOSITION (no state with a full map is built): stage 1 at 4 096 x 32 768 through lvt_amd_reloc_match_device, stages 3 - 5
             at n = 4 096 correspondences (all with a camera-frame point, 40 % gross outliers) and 1 024 hypotheses through lvt_amd_reloc_solve; the host clock
             of the solve entry includes its allocations and copies -- the kernels' own durations come from --kernel-trace
  headline   bench.py --gpus 1 --steps 400 --warmup 20 (frames per second)
  sync       synchronous lvt_track on the same world, p50 of 200 frames in microseconds
"""
import argparse
import json
import os
import statistics as st
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg_match():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import lvt_amd
    rng = np.random.default_rng(0)
    out = {}
    for N, M in ((1052, 844), (4096, 32768)):
        q = torch.from_numpy(rng.integers(0, 256, (N, 32), dtype=np.uint8)).cuda()
        t = torch.from_numpy(rng.integers(0, 256, (M, 32), dtype=np.uint8)).cuda()
        o = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
        us = [lvt_amd.reloc_match_device(q, t, o) for _ in range(25)][5:]
        out[f"{N}x{M}"] = round(st.median(us), 1)
    return out


def _kitti_world():
    sys.path.insert(0, ROOT)
    import lvt_amd
    from lvt_amd.synth import make_world
    world = make_world("kitti", seed=0, scale=1.0)
    prm = lvt_amd.kitti_params(width=world.W, height=world.H, fx=world.fx, fy=world.fy, cx=world.cx, cy=world.cy, baseline=world.baseline)
    return lvt_amd, world, prm


def leg_call():
    import numpy as np
    lvt_amd, world, prm = _kitti_world()
    s = lvt_amd.LvtSystem.create(prm, 1)
    for i in range(8):
        s.track(*world.render_stereo(i))
    flat = np.full((world.H, world.W), 110, np.uint8)
    s.track(flat, flat)
    s.track(*world.render_stereo(12))
    ts = []
    for _ in range(25):
        t0 = time.perf_counter()
        r = s.relocalise(dry_run=1)
        ts.append((time.perf_counter() - t0) * 1e6)
    return {"call_us": round(st.median(ts[5:]), 1), "status": r.status, "n_features": r.n_features, "n_map": r.n_map, "n_corr": r.n_corr,
            "n_refined_inliers": r.n_refined_inliers}


def leg_fullmap():
    sys.path.insert(0, ROOT)
    import numpy as np
    import lvt_amd
    from lvt_amd.synth import noise_frame
    prm = lvt_amd.kitti_params(width=1241, height=376)
    prm.triangulation_policy, prm.staged_threshold, prm.untracked_threshold = 2, 0, 1000
    s = lvt_amd.LvtSystem.create(prm, 1)
    for e in range(12):
        s.track_with_external_corners(*noise_frame(e))
    map_size, state = s.counts()["map_size"], s.get_state()
    flat = np.full((376, 1241), 110, np.uint8)
    s.track(flat, flat)
    lost = s.get_state()
    s.track_with_external_corners(*noise_frame(4))      # (an epoch whose points are in the map: those behind the cut never got in)
    ts = []
    for _ in range(25):
        t0 = time.perf_counter()
        r = s.relocalise(dry_run=1)
        ts.append((time.perf_counter() - t0) * 1e6)
    return {"call_us": round(st.median(ts[5:]), 1), "state_before": state, "state_lost": lost, "map_size": map_size, "status": r.status, "n_features": r.n_features,
            "n_map": r.n_map, "n_matched": r.n_matched, "n_corr": r.n_corr, "n_with_point": r.n_with_point, "n_hyp_inliers": r.n_hyp_inliers,
            "n_refined_inliers": r.n_refined_inliers}


def leg_capacity():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import lvt_amd
    rng = np.random.default_rng(1)
    N, M, n = 4096, 32768, 4096
    q = torch.from_numpy(rng.integers(0, 256, (N, 32), dtype=np.uint8)).cuda()
    t = torch.from_numpy(rng.integers(0, 256, (M, 32), dtype=np.uint8)).cuda()
    o = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    us = [lvt_amd.reloc_match_device(q, t, o) for _ in range(25)][5:]
    prm = lvt_amd.kitti_params()
    ang = 0.3
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    pos = np.array([1.0, -0.2, 2.0])
    pc = np.column_stack([rng.uniform(-12, 12, n), rng.uniform(-3, 3, n), rng.uniform(5, 40, n)])
    X = pc @ R.T + pos
    uv = np.column_stack([prm.fx * pc[:, 0] / pc[:, 2] + prm.cx, prm.fy * pc[:, 1] / pc[:, 2] + prm.cy]) + rng.normal(0, 0.3, (n, 2))
    bad = rng.random(n) < 0.4
    uv[bad] += rng.uniform(30, 200, (int(bad.sum()), 2))
    pcn = pc + rng.normal(0, 0.002, pc.shape)
    pcn[bad] += rng.normal(0, 3.0, (int(bad.sum()), 3))
    cfg = lvt_amd.RelocConfig(n_hypotheses=1024)
    ts = []
    for _ in range(15):
        t0 = time.perf_counter()
        res = lvt_amd.reloc_solve(prm, X, uv.astype(np.float32), pcn, np.ones(n, bool), cfg)[0]
        ts.append((time.perf_counter() - t0) * 1e6)
    return {"match_4096x32768_us": round(st.median(us), 1), "solve_entry_host_us": round(st.median(ts[5:]), 1), "status": res.status,
            "n_hyp_inliers": res.n_hyp_inliers, "n_refined_inliers": res.n_refined_inliers}


def kernel_trace():
    """the `call` and `capacity` legs under rocprofv3 --kernel-trace --stats: calls and average duration of every relocalisation kernel"""
    import csv
    import glob
    import tempfile
    for leg in ("call", "fullmap", "capacity"):
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "reloc", "--", sys.executable, os.path.abspath(__file__), "--leg", leg]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            f = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)
            if out.returncode != 0 or not f:
                raise RuntimeError(f"rocprofv3 on leg {leg} failed:\n{out.stdout[-1500:]}\n{out.stderr[-1500:]}")
            print(f"== {leg}: {out.stdout.strip().splitlines()[-1]}")
            for r in csv.DictReader(open(f[0])):
                if "k_reloc" in r["Name"]:
                    name = r["Name"].replace("void ", "").split("(")[0].replace("lvt::", "")
                    print(f"{name:28s} calls {int(r['Calls']):4d}   average {float(r['AverageNs']) / 1e3:8.1f} us   min {float(r['MinNs']) / 1e3:8.1f}   max {float(r['MaxNs']) / 1e3:8.1f}")


def leg_sync():
    lvt_amd, world, prm = _kitti_world()
    s = lvt_amd.LvtSystem.create(prm, 1)
    frames = [world.render_stereo(i) for i in range(40)]
    ts = []
    for i in range(240):
        L, R = frames[i % 40] if (i // 40) % 2 == 0 else frames[39 - i % 40]      # forth and back: the tracker never leaves the world
        t0 = time.perf_counter()
        s.track(L, R)
        ts.append((time.perf_counter() - t0) * 1e6)
    return {"sync_p50_us": round(st.median(ts[40:]), 1)}


def leg_headline():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "400", "--warmup", "20"], capture_output=True, text=True,
                         timeout=300, env=os.environ)
    return {"fps": json.loads(out.stdout.strip().splitlines()[-1])["value"]}


LEGS = {"match": leg_match, "call": leg_call, "fullmap": leg_fullmap, "capacity": leg_capacity, "sync": leg_sync, "headline": leg_headline}


def child(leg, lib=None, extra=None):
    env = dict(os.environ)
    env.pop("LVT_AMD_LIB", None)
    if lib:
        env["LVT_AMD_LIB"] = lib
    env.update(extra or {})
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], capture_output=True, text=True, timeout=600, env=env)
    if out.returncode != 0:
        raise RuntimeError(f"leg {leg} failed:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-trace", action="store_true")
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(LEGS[a.leg]()))
        return
    if a.kernel_trace:
        kernel_trace()
        return
    for variant, extra in (("lds", {}), ("uniform", {"LVT_AMD_RELOC_MATCH": "uniform"})):
        runs = [child("match", extra=extra) for _ in range(a.repeats)]
        for k in runs[0]:
            v = [r[k] for r in runs]
            print(f"match {variant:8s} {k:12s} median {st.median(v):8.1f} us   repeats {v}")
    runs = [child("call") for _ in range(a.repeats)]
    print("call", {k: runs[0][k] for k in runs[0] if k != "call_us"}, "median", st.median([r["call_us"] for r in runs]), "us   repeats", [r["call_us"] for r in runs])
    runs = [child("fullmap") for _ in range(a.repeats)]
    print("fullmap", {k: runs[0][k] for k in runs[0] if k != "call_us"}, "median", st.median([r["call_us"] for r in runs]), "us   repeats", [r["call_us"] for r in runs])
    runs = [child("capacity") for _ in range(a.repeats)]
    for k in ("match_4096x32768_us", "solve_entry_host_us"):
        print("capacity", k, "median", st.median([r[k] for r in runs]), "  repeats", [r[k] for r in runs], {x: runs[0][x] for x in ("status", "n_hyp_inliers", "n_refined_inliers")})
    for leg, key in (("headline", "fps"), ("sync", "sync_p50_us")):
        got = {"parent": [], "this": []}
        for _ in range(a.repeats):
            if a.parent_lib:
                got["parent"].append(child(leg, lib=os.path.abspath(a.parent_lib))[key])
            got["this"].append(child(leg)[key])
        for who, v in got.items():
            if v:
                print(f"{leg:8s} {who:6s} {key} median {st.median(v):10.1f}   repeats {v}   spread {min(v)} ... {max(v)}")
        if got["parent"]:
            inside = min(got["this"]) <= max(got["parent"]) and min(got["parent"]) <= max(got["this"])
            print(f"{leg:8s} the two sets of repeats {'overlap' if inside else 'DO NOT overlap'}")


if __name__ == "__main__":
    main()
