"""CPU tier: the C-ABI library builds for gfx950 without a GPU, loads, and exports every symbol the headers declare."""
import ctypes
import os
import re

import lvt_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    names = []
    for h in ("lvt_c.h", "lvt_amd_ext.h"):
        txt = open(os.path.join(ROOT, "include", h)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        names += re.findall(r"LVT_API\s+[\w\s\*]+?\b(lvt_\w+)\s*\(", txt)
    return sorted(set(names))


def test_library_exports_every_declared_symbol(hip_lib):
    decl = declared_symbols()
    assert {"lvt_create", "lvt_destroy", "lvt_track", "lvt_track_with_external_corners", "lvt_get_status"} <= set(decl)
    assert {"lvt_amd_pnp", "lvt_amd_pnp_detail", "lvt_amd_pnp_trace", "lvt_amd_motion_predict", "lvt_amd_remap_device"} <= set(decl)     # the stage entry points on caller data
    assert sorted(decl) == sorted(lvt_amd.ABI_SYMBOLS)
    lib = ctypes.CDLL(lvt_amd.LIB_PATH)
    for s in decl:
        assert hasattr(lib, s), f"{s} declared in include/ but not exported"


def test_reference_signatures_are_preserved():
    """the five entry points keep the reference's argument lists (lvt/src/lvt_c.h:57-62)"""
    txt = open(os.path.join(ROOT, "include", "lvt_c.h")).read()
    assert re.search(r"lvt_handle\s+lvt_create\(const char \*config_file_name, int sensor_type\)", txt)
    assert re.search(r"void\s+lvt_track\(lvt_handle vo_system, unsigned char \*left_img, unsigned char \*right_img,\s*int n_rows, int n_cols, double R\[3\]\[3\], double t\[3\]\)", txt)
    assert re.search(r"int\s+lvt_get_status\(lvt_handle vo_system\)", txt)
    assert "typedef void *lvt_handle;" in txt


def test_no_cpu_fallback_without_gpu(hip_lib):
    """without a HIP device lvt_create / lvt_amd_create return NULL: the product never routes through the oracle"""
    import torch
    if torch.cuda.is_available():
        return
    import pytest
    with pytest.raises(RuntimeError):
        lvt_amd.LvtSystem.create(lvt_amd.kitti_params(), 1)


def test_no_handle_is_refused_by_every_frame_and_wait_entry_point(hip_lib):
    """a NULL handle, and memory that is neither a context, a seat nor an automatic handle: every entry point that takes a frame or waits for one
    returns (-1 where it returns an int) with R and t untouched, without a device"""
    import numpy as np
    L = hip_lib.load_library()
    vp = ctypes.c_void_p
    gray = np.zeros((8, 16), np.uint8); d32 = np.zeros((8, 16), np.float32); d16 = np.zeros((8, 16), np.uint16)
    corners = np.zeros((4, 2)); q = np.zeros(4)
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731  (host addresses stand in for device pointers: the handle is refused before any is looked at)
    one, ptr1 = (ctypes.c_int * 1), (vp * 1)
    s = 1.0 / 5000.0
    not_a_handle = np.zeros(64, np.uint64)
    for h in (None, p(not_a_handle)):
        R = np.zeros((3, 3)); t = np.zeros(3); st = np.full(1, 7, np.int32)
        void_calls = {
            "lvt_track": lambda: L.lvt_track(h, p(gray), p(gray), 8, 16, p(R), p(t)),
            "lvt_track_with_external_corners": lambda: L.lvt_track_with_external_corners(h, p(gray), p(gray), 8, 16, p(corners), 4, p(corners), 4, p(R), p(t)),
            "lvt_amd_track_rgbd": lambda: L.lvt_amd_track_rgbd(h, p(gray), p(d32), 8, 16, p(R), p(t)),
            "lvt_amd_track_device": lambda: L.lvt_amd_track_device(h, p(gray), p(gray), 8, 16, 16, p(R), p(t)),
            "lvt_amd_track_device_async": lambda: L.lvt_amd_track_device_async(h, p(gray), p(gray), 8, 16, 16),
            "lvt_amd_wait": lambda: L.lvt_amd_wait(h, p(R), p(t)),
            "lvt_amd_batch_track_device_async": lambda: L.lvt_amd_batch_track_device_async(h, ptr1(gray.ctypes.data), ptr1(gray.ctypes.data), 8, 16, 16),
            "lvt_amd_batch_wait": lambda: L.lvt_amd_batch_wait(h, p(R), p(t), p(st)),
        }
        int_calls = {
            "lvt_get_status": lambda: L.lvt_get_status(h),
            "lvt_amd_wait_status": lambda: L.lvt_amd_wait_status(h, p(R), p(t)),
            "lvt_amd_wait_pose": lambda: L.lvt_amd_wait_pose(h, p(q), p(t)),
            "lvt_amd_track_async": lambda: L.lvt_amd_track_async(h, p(gray), p(gray), 8, 16),
            "lvt_amd_track_rgbd_async": lambda: L.lvt_amd_track_rgbd_async(h, p(gray), p(d32), 8, 16),
            "lvt_amd_batch_track_device_async_mixed": lambda: L.lvt_amd_batch_track_device_async_mixed(h, ptr1(gray.ctypes.data), ptr1(gray.ctypes.data), one(8), one(16), one(16)),
            "lvt_amd_track_rgbd_device_async": lambda: L.lvt_amd_track_rgbd_device_async(h, p(gray), 16, p(d32), 64, 0, 1.0, 8, 16),
            "lvt_amd_track_rgbd_device": lambda: L.lvt_amd_track_rgbd_device(h, p(gray), 16, p(d16), 32, 1, s, 8, 16, p(R), p(t)),
            "lvt_amd_track_rgbd16": lambda: L.lvt_amd_track_rgbd16(h, p(gray), p(d16), s, 8, 16, p(R), p(t)),
            "lvt_amd_track_rgbd16_async": lambda: L.lvt_amd_track_rgbd16_async(h, p(gray), p(d16), s, 8, 16),
            "lvt_amd_batch_track_rgbd_device_async": lambda: L.lvt_amd_batch_track_rgbd_device_async(h, ptr1(gray.ctypes.data), ptr1(d32.ctypes.data), one(8), one(16), one(16), one(64), 0, 1.0),
        }
        assert set(void_calls) | set(int_calls) <= set(lvt_amd.ABI_SYMBOLS)
        # every symbol that tracks or waits is covered (lvt_amd_odometry_update takes an odometry object, not an lvt_handle)
        assert {n for n in lvt_amd.ABI_SYMBOLS if ("track" in n or "wait" in n)} == (set(void_calls) | set(int_calls)) - {"lvt_get_status"}
        L.lvt_get_status.restype = ctypes.c_int
        L.lvt_amd_wait_pose.restype = ctypes.c_int
        for name, call in void_calls.items():
            call()
            assert not R.any() and not t.any() and st[0] == 7, name
        for name, call in int_calls.items():
            assert call() == -1, name
            assert not R.any() and not t.any() and not q.any(), name


def test_motion_predict_refuses_a_null_argument_without_a_device(hip_lib):
    """lvt_amd_motion_predict: -1 for any NULL pointer before the device is touched, the other arrays unchanged"""
    import numpy as np
    L = hip_lib.load_library()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for missing in range(5):
        arrs = [np.full(14, 7.0), np.full(4, 7.0), np.full(3, 7.0), np.full(4, 7.0), np.full(3, 7.0)]
        args = [None if k == missing else p(a) for k, a in enumerate(arrs)]
        assert L.lvt_amd_motion_predict(*args) == -1, missing
        assert all((a == 7.0).all() for a in arrs)


def test_remap_device_refuses_a_null_argument_without_a_device(hip_lib):
    """lvt_amd_remap_device: -1 for any NULL pointer before the device is touched, the sentence with the calling thread, the launch count 0 and the
    destination unchanged (host addresses stand in for device pointers: the call is refused before any is looked at)"""
    import numpy as np
    L = hip_lib.load_library()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for missing in range(4):
        src, m1, m2, dst = np.full(16, 7, np.uint8), np.full(16, 1.0, np.float32), np.full(16, 1.0, np.float32), np.full(16, 7, np.uint8)
        a = [None if k == missing else p(x) for k, x in enumerate((src, m1, m2, dst))]
        n = ctypes.c_int(5)
        assert L.lvt_amd_remap_device(a[0], 4, 4, 4, a[1], a[2], 4, 4, a[3], 4, 0, ctypes.byref(n)) == -1, missing
        assert n.value == 0 and (dst == 7).all() and (src == 7).all()
        assert hip_lib.last_call_error() == "lvt_amd_remap_device: a NULL argument (nothing was launched)", hip_lib.last_call_error()


def test_product_does_not_reference_the_oracle():
    """the oracle is test infrastructure: only tests/ (incl. tests/tools/), __graft_entry__.smoke() and bench.py's cpu_baseline leg
    touch it -- not the package, not the examples, not the developer tools"""
    for top in ("lvt_amd", "examples", "tools", "include"):
        for base, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".cpp", ".sh", ".inc")):
                    txt = open(os.path.join(base, f), errors="ignore").read()
                    assert "pyoracle" not in txt and "lvt_oracle" not in txt and "liblvt_oracle" not in txt and "from oracle" not in txt, (top, f)


def test_lvt_system_facade_compiles_without_opencv_and_eigen(tmp_path):
    """include/lvt_system.h (the reference's C++ API names over the C-ABI) is self-contained: a caller written
    like the reference's examples compiles with neither OpenCV nor Eigen installed, and links against liblvt_c.so"""
    import subprocess
    src = tmp_path / "caller.cpp"
    src.write_text(r'''
#include "lvt_system.h"
#include <cstdio>
int main(int argc, char **argv) {
    lvt_parameters params;                      // defaults of lvt_parameters.cpp:29-52
    if (argc > 1 && !params.init_from_file(argv[1])) return 2;
    params.fx = params.fy = 718.856f; params.cx = 607.19f; params.cy = 185.2f; params.baseline = 0.537f;
    params.img_width = 1241; params.img_height = 376;
    if (params.tracking_radius != 25 || params.staged_threshold != 2 || params.triangulation_policy != lvt_parameters::etriangulation_policy_decreasing_matches) return 3;
    lvt_system *vo = lvt_system::create(params, lvt_system::eSensor_STEREO);   // NULL without a GPU: no CPU fallback
    if (!vo) { std::printf("no device\n"); return 0; }
    std::vector<unsigned char> l(1241 * 376, 7), r(1241 * 376, 7);
    lvt_pose pose = vo->track(lvt_image_view(l.data(), 376, 1241), lvt_image_view(r.data(), 376, 1241));
    lvt_vector3 p = pose.get_position(); lvt_matrix33 R = pose.get_orientation_matrix(); lvt_quaternion q = pose.get_orientation_quaternion();
    lvt_pose_array poses(1); poses[0] = pose;
    std::printf("%g %g %g %d %d\n", p.x() + p(1) + p.z(), R(0, 0), q.w(), (int)vo->get_state(), (int)vo->should_quit());
    lvt_system::destroy(vo);
    return 0;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(lvt_amd.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-DLVT_SYSTEM_NO_OPENCV", "-DLVT_SYSTEM_NO_EIGEN", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           str(src), "-L", libdir, "-llvt_c", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
