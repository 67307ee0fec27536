#!/usr/bin/env python3
"""Dim frames (lvt_amd_set_equalisation): CLAHE inside the feature stage against the route the PARENT commit offered, the caller equalising on one host core
in front of the tracker.  Writes profiles/equalisation.md.

  route    KITTI- (1241 x 376 stereo), EuRoC- (752 x 480 stereo) and TUM-shaped (640 x 480 RGB-D, 16-bit depth) synthetic worlds, every frame dimmed to
           clip(rint(0.12 g + 10)), tiles 8 x 8, clip limit 3.
           new:    a handle with the record set, fed the dimmed frames.
           parent: a compiled restatement of the definition (C++, g++ -O2, one core; checked here against tests/clahe_util.py on one frame) over every image,
                   then the gray entry point.  Planes resident in HBM have no route but through the host: copied back, equalised there, handed in as host frames.
           sync p50 of the synchronising call, frames/s with three host frames in flight, frames/s with planes resident in HBM (three in flight).
  klaunch  the two launches between their HIP events (lvt_amd_profile_read), 100 synchronous frames, with the tables staged in LDS (what ships) and
           gathered through L1 (LVT_AMD_CLAHE_GATHER=l1).
  plain    handles that never set the property, both libraries: the stereo headline route (lvt_amd_track_async, KITTI-shaped page-locked frames), the
           synchronous p50 of lvt_track, the TUM-shaped RGB-D route (lvt_amd_track_rgbd16_async).  The feature must cost them nothing.

--parent-lib names the PARENT commit's liblvt_c.so, built in a worktree of its own; its legs run in child processes of their own (LVT_AMD_LIB) that alternate
with this library's, three times; every figure is the median of the three (min .. max).  Every child runs under its own time limit, warm-up first, profiler
off (but for klaunch); a failing child ends the run (nothing more is started on the GPU).

  python tools/equalisation.py --parent-lib /path/to/parent/liblvt_c.so [--out profiles/equalisation.md] [--resources "..."]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NREND, WARM, DEPTH, TIMED = 24, 15, 3, 200
SCALE = 1.0 / 5000.0
TILES, CLIP = (8, 8), 3.0
SHAPES = ("kitti", "euroc", "tum")

HOST_CLAHE = r"""
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
// the definition of include/lvt_amd_ext.h (DIM frames), restated for one host core; built without FMA contraction
extern "C" void clahe_host(const uint8_t *src, uint8_t *dst, int W, int H, int tx, int ty, float clip_limit) {
    const int Wp = W + (tx - W % tx) % tx, Hp = H + (ty - H % ty) % ty, tw = Wp / tx, th = Hp / ty, area = tw * th;
    const float fa = (float)area, c = clip_limit * fa / 256.0f, scale = 255.0f / fa;
    const int clip = (c >= fa) ? area : std::max((int)c, 1);
    std::vector<uint8_t> lut((size_t)tx * ty * 256);
    for (int j = 0; j < ty; j++)
        for (int i = 0; i < tx; i++) {
            int hist[256] = {0};
            for (int y = j * th; y < (j + 1) * th; y++) {
                const uint8_t *row = src + (size_t)(y >= H ? 2 * (H - 1) - y : y) * W;
                for (int x = i * tw; x < (i + 1) * tw; x++) hist[row[x >= W ? 2 * (W - 1) - x : x]]++;
            }
            int excess = 0;
            for (int k = 0; k < 256; k++)
                if (hist[k] > clip) excess += hist[k] - clip, hist[k] = clip;
            const int batch = excess / 256;
            int residual = excess - 256 * batch;
            for (int k = 0; k < 256; k++) hist[k] += batch;
            if (residual > 0) {
                const int step = std::max(256 / residual, 1);
                for (int k = 0; k < 256 && residual > 0; k += step, residual--) hist[k]++;
            }
            int cum = 0;
            uint8_t *L = &lut[((size_t)j * tx + i) * 256];
            for (int k = 0; k < 256; k++) {
                cum += hist[k];
                L[k] = (uint8_t)std::min(std::max((int)std::nearbyintf((float)cum * scale), 0), 255);
            }
        }
    std::vector<int> x1(W), x2(W);
    std::vector<float> xa(W), xa1(W);
    const float itw = 1.0f / (float)tw, ith = 1.0f / (float)th;
    for (int x = 0; x < W; x++) {
        const float f = (float)x * itw - 0.5f, fl = std::floor(f);
        xa[x] = f - fl, xa1[x] = 1.0f - xa[x];
        x1[x] = std::min(std::max((int)fl, 0), tx - 1) * 256, x2[x] = std::min(std::max((int)fl + 1, 0), tx - 1) * 256;
    }
    for (int y = 0; y < H; y++) {
        const float f = (float)y * ith - 0.5f, fl = std::floor(f), ya = f - fl, ya1 = 1.0f - ya;
        const uint8_t *L1 = &lut[(size_t)std::min(std::max((int)fl, 0), ty - 1) * tx * 256], *L2 = &lut[(size_t)std::min(std::max((int)fl + 1, 0), ty - 1) * tx * 256];
        const uint8_t *s = src + (size_t)y * W;
        uint8_t *d = dst + (size_t)y * W;
        for (int x = 0; x < W; x++) {
            const int v = s[x];
            const float a = (float)L1[x1[x] + v] * xa1[x] + (float)L1[x2[x] + v] * xa[x];
            const float b = (float)L2[x1[x] + v] * xa1[x] + (float)L2[x2[x] + v] * xa[x];
            d[x] = (uint8_t)std::min(std::max((int)std::nearbyintf(a * ya1 + b * ya), 0), 255);
        }
    }
}
"""


def pingpong(k):
    p = 2 * (NREND - 1)
    k %= p
    return k if k < NREND else p - k


def host_clahe():
    """the restatement above, compiled as the examples are (g++ -O2), and checked against tests/clahe_util.py"""
    import numpy as np
    d = tempfile.mkdtemp(prefix="lvt_clahe_")
    src, lib = os.path.join(d, "clahe_host.cpp"), os.path.join(d, "libclahe_host.so")
    with open(src, "w") as f:
        f.write(HOST_CLAHE)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src])
    fn = C.CDLL(lib).clahe_host
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import clahe_util as CL
    img = np.random.default_rng(0).integers(0, 60, (83, 97), dtype=np.uint8)
    out = np.zeros_like(img)
    fn(img.ctypes.data, out.ctypes.data, 97, 83, 8, 8, 3.0)
    assert np.array_equal(out, CL.clahe(img, (8, 8), 3.0)), "the compiled restatement differs from tests/clahe_util.py"

    def run(a, out):
        fn(a.ctypes.data, out.ctypes.data, a.shape[1], a.shape[0], TILES[0], TILES[1], CLIP)
        return out
    return run


def dim_t(t):
    import torch
    return torch.clamp(torch.round(0.12 * t.double() + 10.0), 0, 255).to(torch.uint8)


def world_frames(lvt, kind):
    """(params, sensor, dimmed device frames [(left, right) | (gray, depth int16)]) of a synthetic world of that shape"""
    import torch
    from lvt_amd.synth import make_world
    w = make_world(kind, seed=0)
    if kind == "tum":
        prm = lvt.tum_params(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy)
        fr = []
        for i in range(NREND):
            g, d = w.render_rgbd_torch(i, device="cuda")
            fr.append((dim_t(g).contiguous(), torch.clamp(torch.round(d.double() * 5000.0), 0, 65535).to(torch.int32).to(torch.int16).contiguous()))
        return w, prm, 2, fr
    mk = lvt.kitti_params if kind == "kitti" else lvt.euroc_params
    prm = mk(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy, baseline=w.baseline)
    fr = []
    for i in range(NREND):
        t = w.render_stereo_torch(i, device="cuda")
        fr.append((dim_t(t[0]).contiguous(), dim_t(t[1]).contiguous()))
    torch.cuda.synchronize()
    return w, prm, 1, fr


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


def timed_sync(call):
    k = 0
    for _ in range(WARM):
        call(k); k += 1
    dts = []
    for _ in range(TIMED):
        t0 = time.perf_counter(); call(k); dts.append(time.perf_counter() - t0); k += 1
    return round(1e6 * statistics.median(dts), 1)


def leg_route(lvt, kind, role):
    import numpy as np
    import torch
    w, prm, sensor, dev = world_frames(lvt, kind)
    H, W = w.H, w.W
    pitch = (W + 63) // 64 * 64
    new = role == "new"
    eq = None if new else host_clahe()
    host = [tuple(x.cpu().numpy() for x in f) for f in dev]
    if sensor == 2:
        host = [(g, d.view(np.uint16)) for g, d in host]
    ring = [tuple(np.zeros((H, W), np.uint8) for _ in range(2)) for _ in range(DEPTH + 2)]   # the parent's route: equalised frames, alive while in flight

    def create():
        h = lvt.LvtSystem.create(prm, sensor)
        if new:
            assert h.set_equalisation(lvt.Equalisation(TILES, CLIP)) == 0, h.last_error()
        return h

    def frame(k, src=None):
        f = (src or host)[pingpong(k)]
        if new:
            return f
        r = ring[k % len(ring)]
        if sensor == 2:
            return eq(f[0], r[0]), f[1]
        return eq(f[0], r[0]), eq(f[1], r[1])

    def track(h, f):
        return h.track(f[0], f[1], depth_scale=SCALE) if sensor == 2 else h.track(*f)

    def track_async(h, f):
        rc = h.track_async(f[0], f[1], depth_scale=SCALE) if sensor == 2 else h.track_async(*f)
        assert rc == 0, h.last_error()
    out = {}
    h = create()
    out["sync_p50_us"] = timed_sync(lambda k: track(h, frame(k)))
    bad = int(h.get_state() != 2)
    wait = lambda: int(h.wait_status()[2] != 2)   # noqa: E731
    out["async_fps"], lost = timed_async(lambda k: track_async(h, frame(k)), wait, TIMED)
    bad += lost
    err = h.last_error()
    h.close()
    # planes resident in HBM (pitched, as a decoder or a camera driver leaves them)
    planes = [tuple(torch.zeros((H, pitch), dtype=torch.uint8, device="cuda") for _ in range(1 if sensor == 2 else 2)) for _ in range(NREND)]
    for p, f in zip(planes, dev):
        for a, b in zip(p, f):
            a[:, :W] = b
    torch.cuda.synchronize()
    h = create()

    def enq_dev(k):
        i = pingpong(k)
        if new:
            if sensor == 2:
                assert h.track_rgbd_device_async(planes[i][0].data_ptr(), dev[i][1].data_ptr(), H, W, pitch, 2 * W, lvt.DEPTH_U16, SCALE) == 0, h.last_error()
            else:
                h.track_device_async(planes[i][0].data_ptr(), planes[i][1].data_ptr(), H, W, pitch)
            return
        back = tuple(np.ascontiguousarray(p[:, :W].cpu().numpy()) for p in planes[i])    # no route but through the host
        r = ring[k % len(ring)]
        if sensor == 2:
            track_async(h, (eq(back[0], r[0]), host[i][1]))
        else:
            track_async(h, (eq(back[0], r[0]), eq(back[1], r[1])))
    out["hbm_async_fps"], lost = timed_async(enq_dev, wait, TIMED)
    out["frames_not_tracking"], out["error"] = bad + lost, err + h.last_error()
    h.close()
    if not new:
        dts = []
        for k in range(50):
            t0 = time.perf_counter(); eq(host[k % NREND][0], ring[0][0]); dts.append(time.perf_counter() - t0)
        out["host_clahe_us_per_image"] = round(1e6 * statistics.median(dts), 1)
    return out


def leg_klaunch(lvt, kind):
    w, prm, sensor, dev = world_frames(lvt, kind)
    host = [tuple(x.cpu().numpy() for x in f) for f in dev]
    if sensor == 2:
        import numpy as np
        host = [(g, d.view(np.uint16)) for g, d in host]
    h = lvt.LvtSystem.create(prm, sensor)
    assert h.set_equalisation(lvt.Equalisation(TILES, CLIP)) == 0, h.last_error()
    track = (lambda f: h.track(f[0], f[1], depth_scale=SCALE)) if sensor == 2 else (lambda f: h.track(*f))
    for k in range(WARM):
        track(host[pingpong(k)])
    h.profile_enable(True)
    for k in range(100):
        track(host[pingpong(WARM + k)])
    prof = {n: (ms, calls) for n, ms, calls in h.profile_read()}
    out = {n + "_us": round(1e3 * prof[n][0] / max(prof[n][1], 1), 2) for n in ("k_clahe_lut", "k_clahe_apply")}
    out.update(calls=prof["k_clahe_lut"][1], error=h.last_error(), frames_not_tracking=int(h.get_state() != 2))
    h.close()
    return out


def leg_plain(lvt):
    import numpy as np
    import torch
    from lvt_amd.synth import make_world
    out = {}
    w = make_world("kitti", seed=0)
    prm = lvt.kitti_params(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy, baseline=w.baseline)
    keep = [w.render_stereo_torch(i, device="cuda").cpu().pin_memory() for i in range(NREND)]
    host = [(t[0].numpy(), t[1].numpy()) for t in keep]
    h = lvt.LvtSystem.create(prm, 1)
    wait = lambda: int(h.wait_status()[2] != 2)   # noqa: E731
    out["stereo_async_fps"], lost = timed_async(lambda k: h.track_async(*host[pingpong(k)]), wait, 300)
    out["stereo_sync_p50_us"] = timed_sync(lambda k: h.track(*host[pingpong(k)]))
    bad, err = lost + int(h.get_state() != 2), h.last_error()
    h.close()
    w = make_world("tum", seed=0)
    prm = lvt.tum_params(width=w.W, height=w.H, fx=w.fx, fy=w.fy, cx=w.cx, cy=w.cy)
    fr = []
    for i in range(NREND):
        g, d = w.render_rgbd_torch(i, device="cuda")
        fr.append((g.cpu().numpy(), torch.clamp(torch.round(d.double() * 5000.0), 0, 65535).to(torch.int32).cpu().numpy().astype(np.uint16)))
    h = lvt.LvtSystem.create(prm, 2)
    out["rgbd_async_fps"], lost = timed_async(lambda k: h.track_async(*fr[pingpong(k)], depth_scale=SCALE), wait, 300)
    out["frames_not_tracking"], out["error"] = bad + lost, err + h.last_error()
    h.close()
    return out


def run_child(args, lib=None, limit=300, env_extra=None):
    env = dict(os.environ)
    if lib:
        env["LVT_AMD_LIB"] = lib
    env.update(env_extra or {})
    out = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=limit, env=env, cwd=ROOT)
    if out.returncode != 0:   # a failed leg ends the run: nothing more is started on the GPU
        print(json.dumps({"leg": args, "failed": out.returncode, "stderr": out.stderr[-3000:]}), flush=True)
        raise SystemExit(1)
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps({"leg": args[1:], "lib": lib or "this checkout", "env": env_extra or {}, "result": r}), flush=True)
    return r


def fmt(v, digits=0):
    return f"{statistics.median(v):.{digits}f} ({min(v):.{digits}f} .. {max(v):.{digits}f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="liblvt_c.so of the parent commit, built in a worktree of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equalisation.md"))
    ap.add_argument("--resources", default="", help="the compiler's resource report of the two kernels, for the report")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--role", default="new", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, ROOT)
        import lvt_amd as lvt
        what, _, kind = a.child.partition(":")
        r = leg_route(lvt, kind, a.role) if what == "route" else leg_klaunch(lvt, kind) if what == "klaunch" else leg_plain(lvt)
        print(json.dumps(r), flush=True)
        return
    me = os.path.abspath(__file__)
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    route = {(k, r): [] for k in SHAPES for r in ("new", "parent")}
    plain = {"new": [], "parent": []}
    kl = {(k, v): [] for k in SHAPES for v in ("lds", "l1")}
    for rep in range(a.repeats):   # the routes and the two libraries alternate
        for kind in SHAPES:
            route[(kind, "parent")].append(run_child([me, "--child", "route:" + kind, "--role", "parent"], lib=parent, limit=400))
            route[(kind, "new")].append(run_child([me, "--child", "route:" + kind, "--role", "new"], limit=400))
            kl[(kind, "lds")].append(run_child([me, "--child", "klaunch:" + kind], limit=200))
            kl[(kind, "l1")].append(run_child([me, "--child", "klaunch:" + kind], limit=200, env_extra={"LVT_AMD_CLAHE_GATHER": "l1"}))
        if parent:
            plain["parent"].append(run_child([me, "--child", "plain"], lib=parent, limit=300))
        plain["new"].append(run_child([me, "--child", "plain"], limit=300))

    who = "the parent commit's library" if parent else "this commit's library: the parent commit itself was not measured"
    L = ["# Dim frames: CLAHE equalisation inside the feature stage", "",
         "Written by `tools/equalisation.py`.  Synthetic worlds (seed 0) of KITTI (1241 x 376 stereo), EuRoC (752 x 480 stereo) and TUM (640 x 480 RGB-D, 16-bit depth)",
         "shape, every frame dimmed to clip(rint(0.12 g + 10)); tiles 8 x 8, clip limit 3.  `sync p50`: host clock around the synchronising call, median of",
         f"{TIMED} calls.  `async`: frames over wall time, {TIMED} frames, three in flight.  Every figure: median of {a.repeats} alternated repeats (min .. max).",
         "`new`: a handle with the record set, fed the dimmed frames.  `caller equalises`: the parent's route on " + who + " -- a compiled restatement of the",
         "definition (C++, g++ -O2, one host core) over every image, then the gray entry point; planes resident in HBM are copied back to the host first, for the",
         "parent has no other route for them.", "",
         "| shape | row | new | caller equalises | new at least as fast |", "|---|---|---|---|---|"]
    for kind in SHAPES:
        for key, title, lower in (("sync_p50_us", "synchronous p50 [us]", True), ("async_fps", "host frames, three in flight [frames/s]", False),
                                  ("hbm_async_fps", "planes resident in HBM, three in flight [frames/s]", False)):
            nv, pv = [r[key] for r in route[(kind, "new")]], [r[key] for r in route[(kind, "parent")]]
            ok = statistics.median(nv) <= statistics.median(pv) if lower else statistics.median(nv) >= statistics.median(pv)
            bad = sum(r["frames_not_tracking"] for r in route[(kind, "new")] + route[(kind, "parent")])
            L.append(f"| {kind} | {title} | {fmt(nv, 1)} | {fmt(pv, 1)} | {'yes' if ok else 'NO'} |" + (f" frames not tracking: {bad}" if bad else ""))
    L += [""]
    for kind in SHAPES:
        L.append(f"- the host restatement over one {kind}-shaped image on one core: {fmt([r['host_clahe_us_per_image'] for r in route[(kind, 'parent')]], 1)} us.")
    L += ["", "## The two launches", "",
          "Between their HIP events, as `lvt_amd_profile_read` reports them (each figure includes the event pair's own few microseconds), mean over 100 synchronous",
          "frames per repeat.  A stereo launch holds both eyes.  `LDS`: k_clahe_apply stages the tables of a workgroup's tile rows in LDS (what ships);",
          "`L1`: it gathers them from the table buffer (`LVT_AMD_CLAHE_GATHER=l1`).", "",
          "| shape | k_clahe_lut [us] | k_clahe_apply, LDS [us] | k_clahe_apply, L1 [us] |", "|---|---|---|---|"]
    for kind in SHAPES:
        L.append(f"| {kind} | {fmt([r['k_clahe_lut_us'] for r in kl[(kind, 'lds')]], 2)} | {fmt([r['k_clahe_apply_us'] for r in kl[(kind, 'lds')]], 2)} | "
                 f"{fmt([r['k_clahe_apply_us'] for r in kl[(kind, 'l1')]], 2)} |")
    L += ["", f"- compiler's resource report: {a.resources or 'see DESIGN.md'}", "", "## No cost to handles that never set the property", ""]
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
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
