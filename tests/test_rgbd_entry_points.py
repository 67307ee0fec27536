"""CPU tier of the RGB-D entry points (device-resident planes, 16-bit depth, lock-step batches): every new symbol is declared in the extension
header, listed in lvt_amd.ABI_SYMBOLS and exported by liblvt_c.so, and each call returns -1 on a NULL handle without touching a device."""
import ctypes as C
import os
import re

import numpy as np

import lvt_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["lvt_amd_track_rgbd_device_async", "lvt_amd_track_rgbd_device", "lvt_amd_track_rgbd16", "lvt_amd_track_rgbd16_async",
               "lvt_amd_batch_track_rgbd_device_async"]


def _lib():
    if not os.path.exists(lvt_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return lvt_amd.load_library()


def test_declared_listed_exported():
    text = open(os.path.join(ROOT, "include", "lvt_amd_ext.h")).read()
    lib = C.CDLL(lvt_amd.LIB_PATH) if os.path.exists(lvt_amd.LIB_PATH) else _lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"LVT_API\s+int\s+" + name + r"\s*\(", text), f"{name} is not declared in lvt_amd_ext.h"
        assert name in lvt_amd.ABI_SYMBOLS, f"{name} is not in ABI_SYMBOLS"
        assert hasattr(lib, name), f"liblvt_c.so does not export {name}"
    m = re.search(r"enum\s*\{\s*LVT_AMD_DEPTH_F32\s*=\s*0\s*,\s*LVT_AMD_DEPTH_U16\s*=\s*1\s*\}", text)
    assert m, "the depth formats are not declared"
    assert (lvt_amd.DEPTH_F32, lvt_amd.DEPTH_U16) == (0, 1)


def test_null_handle_is_refused_without_a_device():
    L = _lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"liblvt_c.so does not export {name}"
    gray = np.zeros((8, 16), np.uint8); d32 = np.zeros((8, 16), np.float32); d16 = np.zeros((8, 16), np.uint16)
    R = np.zeros((3, 3)); t = np.zeros(3)
    vp = C.c_void_p
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731  (host addresses stand in for device pointers: a NULL handle is refused before any is looked at)
    s = 1.0 / 5000.0
    assert L.lvt_amd_track_rgbd_device_async(None, p(gray), 16, p(d32), 64, 0, 1.0, 8, 16) == -1
    assert L.lvt_amd_track_rgbd_device(None, p(gray), 16, p(d16), 32, 1, s, 8, 16, p(R), p(t)) == -1
    assert L.lvt_amd_track_rgbd16(None, p(gray), p(d16), s, 8, 16, p(R), p(t)) == -1
    assert L.lvt_amd_track_rgbd16_async(None, p(gray), p(d16), s, 8, 16) == -1
    one = (C.c_int * 1)
    assert L.lvt_amd_batch_track_rgbd_device_async(None, (vp * 1)(gray.ctypes.data), (vp * 1)(d32.ctypes.data), one(8), one(16), one(16), one(64), 0, 1.0) == -1
    assert not R.any() and not t.any()
