#!/usr/bin/env python3
"""Lens models (lvt_amd_rectifier_create_lens) and raw frames of another size than the tracker's: what they cost, what they cost callers that do not use
them, and what they save against the only route the PARENT commit offers a fisheye camera.  Writes profiles/lens_models.md.

  create      host clock around the creating call (it synchronises: maps built, fixed-point form made), median of 9 calls: RADTAN (12 coefficients) and
              FISHEYE at 752 x 480 and at 1024 x 1024 -> 512 x 512, lvt_amd_rectifier_create at 752 x 480.  A one-time cost: reported, not gated.
  remap       k_rectify_frames between its HIP events (lvt_amd_profile_*), one stereo pair per launch, 100 frames through lvt_amd_track_device: a FISHEYE pair
              rectified to 752 x 480 from a source of the same size, of 4/3 the size (1003 x 640) and of twice the size (1504 x 960).
  plain       callers that do NOT use the feature, this library and the parent's alternated: a plain handle (rectified EuRoC-shaped frames in HBM, three in
              flight, frames/s; synchronous lvt_track p50) and a handle with lvt_amd_rectifier_create's rectifiers on raw frames (three in flight); and the
              headline of `python bench.py --gpus 1`.
  fisheye     a 1024 x 1024 fisheye pair tracked at 512 x 512 (TUM-VI-shaped), synchronous p50 and three frames in flight, host frames.
              new: rectifiers of lvt_amd_rectifier_create_lens attached, raw frames handed in.  parent route: the caller remaps both images on one host
              core with a compiled restatement of the remap (tools/lens_remap_host.c, -O2) under maps it built itself, then the gray entry point.

--parent-lib names the PARENT commit's liblvt_c.so, built in a worktree of its own; its legs run in child processes of their own (LVT_AMD_LIB) that
alternate with this library's, three times; every figure is the median of the three (min .. max).  Every leg is a child process under its own time
limit, warm-up first; a failing leg ends the run (nothing more is started on the GPU).

  python tools/lens_models.py --parent-lib /path/to/parent/liblvt_c.so [--out profiles/lens_models.md] [--no-bench] [--map-diffs "0 of 198 052"]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NREND, WARM, DEPTH, TIMED = 24, 20, 3, 300
EYE3 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
P_NEW = [435.2046959714599, 0, 367.4517211914062, 0, 435.2046959714599, 252.2008514404297, 0, 0, 1]
PINCUSHION = [0.12, 0.02, 2e-4, -1e-4, 0.0]
RADTAN12 = [0.12, 0.02, 2e-4, -1e-4, 0.01, 0.05, 0.01, 0.002, 1e-3, -5e-4, 5e-4, 1e-3]
FISHEYE_D = [-0.02, 0.004, -0.001, 0.0002]


def pingpong(k):
    p = 2 * (NREND - 1)
    k %= p
    return k if k < NREND else p - k


def world_frames(size, seed=1):
    """(world, frames): NREND stereo pairs of the synthetic EuRoC world rendered at `size`, in HBM, pitch = width rounded up to 64"""
    import torch
    from lvt_amd.synth import make_world
    w = make_world("euroc", seed=seed, size=size)
    pitch = (w.W + 63) // 64 * 64
    fr = torch.zeros((NREND, 2, w.H, pitch), dtype=torch.uint8, device="cuda")
    for i in range(NREND):
        a, b = w.render_stereo_torch(i, device="cuda")
        fr[i, 0, :, :w.W] = a; fr[i, 1, :, :w.W] = b
    torch.cuda.synchronize()
    return w, fr, pitch


def params_for(lvt, w):
    prm = lvt.euroc_params()
    prm.fx, prm.fy, prm.cx, prm.cy, prm.baseline = w.fx, w.fy, w.cx, w.cy, w.baseline
    prm.img_width, prm.img_height = w.W, w.H
    return prm


def world_K(w):
    return [w.fx, 0.0, w.cx, 0.0, w.fy, w.cy, 0.0, 0.0, 1.0]


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


def timed_sync(call, n):
    k = 0
    for _ in range(WARM):
        call(k); k += 1
    dts = []
    for _ in range(n):
        t0 = time.perf_counter(); call(k); dts.append(time.perf_counter() - t0); k += 1
    return round(1e6 * statistics.median(dts), 1)


def leg_create(lvt):
    out = {}

    def med(make):
        ts = []
        for _ in range(10):
            t0 = time.perf_counter(); r = make(); ts.append(time.perf_counter() - t0); r.close()
        return round(1e3 * statistics.median(ts[1:]), 3)
    K = [458.654, 0.0, 367.215, 0.0, 457.296, 248.375, 0.0, 0.0, 1.0]
    out["old_752x480_ms"] = med(lambda: lvt.Rectifier(K, PINCUSHION, EYE3, P_NEW, 752, 480))
    K2 = [380.0, 0.0, 511.5, 0.0, 380.0, 511.5, 0.0, 0.0, 1.0]
    P2 = [190.0, 0.0, 255.5, 0.0, 190.0, 255.5, 0.0, 0.0, 1.0]
    for name, model, D in (("radtan", 0, RADTAN12), ("fisheye", 1, FISHEYE_D)):
        out[f"{name}_752x480_ms"] = med(lambda: lvt.Rectifier.from_lens(lvt.Lens(model, 752, 480, K, D), EYE3, P_NEW, 752, 480))
        out[f"{name}_1024x1024_to_512x512_ms"] = med(lambda: lvt.Rectifier.from_lens(lvt.Lens(model, 1024, 1024, K2, D), EYE3, P2, 512, 512))
    return out


def leg_remap(lvt):
    """k_rectify_frames' own time for one pair, by the size of its source"""
    out = {}
    wd, _, _ = world_frames((752, 480))
    prm = params_for(lvt, wd)
    for tag, size in (("same_size", (752, 480)), ("four_thirds", (1003, 640)), ("twice", (1504, 960))):
        ws, fr, pitch = world_frames(size)
        r = lvt.Rectifier.from_lens(lvt.Lens(1, ws.W, ws.H, world_K(ws), FISHEYE_D), EYE3, world_K(wd), wd.W, wd.H)
        h = lvt.LvtSystem.create(prm, 1)
        assert h.set_rectifiers(r, r) == 0, h.last_error()
        for k in range(WARM):
            h.track_device(fr[pingpong(k), 0].data_ptr(), fr[pingpong(k), 1].data_ptr(), ws.H, ws.W, pitch)
        h.profile_enable(True)
        for k in range(100):
            h.track_device(fr[pingpong(k), 0].data_ptr(), fr[pingpong(k), 1].data_ptr(), ws.H, ws.W, pitch)
        prof = {n: (ms, calls) for n, ms, calls in h.profile_read()}
        ms, calls = prof["k_rectify_frames"]
        out[tag] = dict(source=f"{ws.W} x {ws.H}", us_per_launch=round(1e3 * ms / calls, 2), launches=calls, state=h.get_state(), error=h.last_error())
        h.close()
    return out


def leg_plain(lvt):
    """callers that do not use the feature (runs under either library)"""
    import torch
    w, raw, pitch = world_frames((752, 480))
    prm = params_for(lvt, w)
    K = world_K(w)
    old = lvt.Rectifier(K, PINCUSHION, EYE3, K, w.W, w.H)
    rect = torch.zeros_like(raw)
    for i in range(NREND):
        for e in (0, 1):
            assert old.rectify_device(raw[i, e].data_ptr(), pitch, rect[i, e].data_ptr(), pitch) == 0
    torch.cuda.synchronize()
    out = {}
    h = lvt.LvtSystem.create(prm, 1)
    fps, lost = timed_async(lambda k: h.track_device_async(rect[pingpong(k), 0].data_ptr(), rect[pingpong(k), 1].data_ptr(), w.H, w.W, pitch),
                            lambda: int(h.wait_status()[2] != 2), TIMED)
    out["plain_async_fps"] = fps
    host = [(rect[i, 0, :, :w.W].contiguous().cpu().numpy(), rect[i, 1, :, :w.W].contiguous().cpu().numpy()) for i in range(NREND)]
    out["plain_sync_p50_us"] = timed_sync(lambda k: h.track(*host[pingpong(k)]), TIMED)
    out["plain_not_tracking"], out["plain_error"] = lost + int(h.get_state() != 2), h.last_error()
    h.close()
    h = lvt.LvtSystem.create(prm, 1)
    assert h.set_rectifiers(old, old) == 0, h.last_error()
    fps, lost = timed_async(lambda k: h.track_device_async(raw[pingpong(k), 0].data_ptr(), raw[pingpong(k), 1].data_ptr(), w.H, w.W, pitch),
                            lambda: int(h.wait_status()[2] != 2), TIMED)
    out["old_style_async_fps"], out["old_style_not_tracking"], out["old_style_error"] = fps, lost, h.last_error()
    h.close()
    return out


def host_remap():
    """tools/lens_remap_host.c compiled (-O2) into a temporary directory: the remap on one host core"""
    import ctypes as C
    import tempfile
    d = tempfile.mkdtemp(prefix="lens_remap_")
    so = os.path.join(d, "liblens_remap_host.so")
    subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "lens_remap_host.c"), "-lm"])
    fn = C.CDLL(so).lens_remap_host
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    fn.restype = None
    return fn


def leg_fisheye(lvt, attached):
    """1024 x 1024 -> 512 x 512, host frames.  attached: this library's route; otherwise the parent's: maps by the caller, remap on one host core"""
    import numpy as np
    ws, fr, _ = world_frames((1024, 1024))
    wd, _, _ = world_frames((512, 512))
    prm = params_for(lvt, wd)
    host = [(fr[i, 0, :, :ws.W].contiguous().cpu().numpy(), fr[i, 1, :, :ws.W].contiguous().cpu().numpy()) for i in range(NREND)]
    h = lvt.LvtSystem.create(prm, 1)
    if attached:
        r = lvt.Rectifier.from_lens(lvt.Lens(1, ws.W, ws.H, world_K(ws), FISHEYE_D), EYE3, world_K(wd), wd.W, wd.H)
        assert h.set_rectifiers(r, r) == 0, h.last_error()
        frame = lambda k: host[pingpong(k)]
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import lens_util
        remap = host_remap()
        m1, m2 = (np.ascontiguousarray(m) for m in lens_util.lens_maps(1, world_K(ws), FISHEYE_D, EYE3, world_K(wd), wd.W, wd.H))
        ring = [(np.zeros((wd.H, wd.W), np.uint8), np.zeros((wd.H, wd.W), np.uint8)) for _ in range(DEPTH + 2)]

        def frame(k):   # (the rectified pair stays alive while its frame is in flight)
            out = ring[k % len(ring)]
            for src, dst in zip(host[pingpong(k)], out):
                remap(lvt._p(src), ws.W, ws.H, ws.W, lvt._p(m1), lvt._p(m2), wd.W, wd.H, lvt._p(dst))
            return out
    out = {"sync_p50_us": timed_sync(lambda k: h.track(*frame(k)), 150)}
    out["state_after_sync"] = h.get_state()

    def enq(k):
        a, b = frame(k)
        assert h.track_async(a, b) == 0, h.last_error()
    fps, lost = timed_async(enq, lambda: int(h.wait_status()[2] != 2), 150)
    out["async_fps"], out["not_tracking"], out["error"] = fps, lost, h.last_error()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_models.md"))
    ap.add_argument("--no-bench", action="store_true", help="skip the bench.py headline")
    ap.add_argument("--map-diffs", default="", help="the count tests/test_gpu_lens_models.py printed for the FISHEYE maps, quoted in the report")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, ROOT)
        import lvt_amd as lvt
        legs = {"create": lambda: leg_create(lvt), "remap": lambda: leg_remap(lvt), "plain": lambda: leg_plain(lvt),
                "fisheye_new": lambda: leg_fisheye(lvt, True), "fisheye_parent": lambda: leg_fisheye(lvt, False)}
        print(json.dumps(legs[a.child]()), flush=True)
        return
    me = os.path.abspath(__file__)
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    res = {k: [] for k in ("create", "remap", "plain_new", "plain_parent", "fisheye_new", "fisheye_parent", "bench_new", "bench_parent")}
    bench = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "300", "--warmup", "20", "--no-cpu"]
    for rep in range(3):   # the two libraries alternate, three times
        if parent:
            res["plain_parent"].append(run_child([me, "--child", "plain"], lib=parent))
        res["plain_new"].append(run_child([me, "--child", "plain"]))
        res["fisheye_parent"].append(run_child([me, "--child", "fisheye_parent"], lib=parent))
        res["fisheye_new"].append(run_child([me, "--child", "fisheye_new"]))
        res["create"].append(run_child([me, "--child", "create"]))
        res["remap"].append(run_child([me, "--child", "remap"]))
        if not a.no_bench:
            if parent:
                res["bench_parent"].append(run_child(bench, lib=parent, limit=420))
            res["bench_new"].append(run_child(bench, limit=420))

    who = "the parent commit's library" if parent else "THIS commit's library (no --parent-lib: the parent commit itself was not measured)"
    L = ["# Lens models: rational and fisheye rectifiers, raw frames of any size", "",
         "Written by `tools/lens_models.py` on one MI355X.  Every figure: median of three alternated repeats (min .. max).", ""]
    if a.map_diffs:
        L += [f"FISHEYE maps against the numpy restatement (`tests/test_gpu_lens_models.py`, four shapes): {a.map_diffs} entries differ.", ""]
    L += ["## Creating a rectifier (one-time; the call synchronises) [ms]", "", "| rectifier | ms |", "|---|---|"]
    for key, title in (("old_752x480_ms", "`lvt_amd_rectifier_create`, 752 x 480"), ("radtan_752x480_ms", "RADTAN (12 coefficients), 752 x 480"),
                       ("fisheye_752x480_ms", "FISHEYE, 752 x 480"), ("radtan_1024x1024_to_512x512_ms", "RADTAN, 1024 x 1024 -> 512 x 512"),
                       ("fisheye_1024x1024_to_512x512_ms", "FISHEYE, 1024 x 1024 -> 512 x 512")):
        L.append(f"| {title} | {fmt([r[key] for r in res['create']], 3)} |")
    L += ["", "## `k_rectify_frames`, one pair to 752 x 480, between its HIP events [us per launch]", "", "| source | us |", "|---|---|"]
    for tag in ("same_size", "four_thirds", "twice"):
        L.append(f"| {res['remap'][0][tag]['source']} | {fmt([r[tag]['us_per_launch'] for r in res['remap']], 2)} |")
    L += ["", "## Callers that do not use the feature", "", f"`parent`: {who}.", "", "| row | this commit | spread | parent | spread | difference of the medians inside the spreads |", "|---|---|---|---|---|---|"]

    def ab(title, new, par):
        if not new:
            return
        sn = max(new) - min(new)
        if par:
            sp = max(par) - min(par)
            inside = abs(statistics.median(new) - statistics.median(par)) <= max(sn, sp)
            L.append(f"| {title} | {fmt(new)} | {sn:.1f} | {fmt(par)} | {sp:.1f} | {'yes' if inside else 'NO'} |")
        else:
            L.append(f"| {title} | {fmt(new)} | {sn:.1f} | not measured | | |")
    for key, title in (("plain_async_fps", "plain handle, planes in HBM, three in flight [frames/s]"), ("plain_sync_p50_us", "plain handle, synchronous `lvt_track` p50 [us]"),
                       ("old_style_async_fps", "`lvt_amd_rectifier_create` rectifiers attached, raw planes in HBM, three in flight [frames/s]")):
        ab(title, [r[key] for r in res["plain_new"]], [r[key] for r in res["plain_parent"]])
    ab("`python bench.py --gpus 1 --steps 300 --warmup 20 --no-cpu` headline [frames/s]", [r["value"] for r in res["bench_new"] if "value" in r],
       [r["value"] for r in res["bench_parent"] if "value" in r])
    bad = sum(r["plain_not_tracking"] + r["old_style_not_tracking"] for r in res["plain_new"] + res["plain_parent"])
    L += ["", f"Frames not TRACKING in these legs: {bad}.", "",
          "## A 1024 x 1024 fisheye pair tracked at 512 x 512, host frames", "",
          f"`parent route` (on {who}): the caller remaps both images on one host core (`tools/lens_remap_host.c` compiled with -O2, maps built by the caller), "
          "then `lvt_track` / `lvt_amd_track_async` on the rectified pair.  `new`: the rectifiers attached, raw frames handed in.", "",
          "| row | new | parent route |", "|---|---|---|",
          f"| synchronous p50 [us] | {fmt([r['sync_p50_us'] for r in res['fisheye_new']])} | {fmt([r['sync_p50_us'] for r in res['fisheye_parent']])} |",
          f"| three frames in flight [frames/s] | {fmt([r['async_fps'] for r in res['fisheye_new']])} | {fmt([r['async_fps'] for r in res['fisheye_parent']])} |", "",
          f"Frames not TRACKING: new {sum(r['not_tracking'] for r in res['fisheye_new'])}, parent route {sum(r['not_tracking'] for r in res['fisheye_parent'])}."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
