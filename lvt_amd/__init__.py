"""lvt_amd -- MI355X-native drop-in for the per-frame tracking hot path of SAR-Research-Lab/lvt.

The product is the C-ABI shared library `lvt_amd/lib/liblvt_c.so` (hand-written gfx950 HIP kernels
behind the reference's own `lvt_c` boundary, see include/lvt_c.h).  This module is the thin Python
mirror of the reference's `lvt_system` interface (lvt/src/lvt_system.h:57-70) used by the tests and
bench harness: same operation names, same argument meaning, same "silent failure" semantics.

There is NO CPU fallback: importing works anywhere (so the CPU test tier can check the exported symbols),
but creating a system without the HIP library or without a GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .params import LvtParameters, ParamsPOD, kitti_params, euroc_params, tum_params  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LVT_AMD_LIB") or os.path.join(_HERE, "lib", "liblvt_c.so")  # override: kernel A/B experiments

# every symbol include/lvt_c.h and include/lvt_amd_ext.h declare
ABI_SYMBOLS = [
    "lvt_create", "lvt_destroy", "lvt_track", "lvt_track_with_external_corners", "lvt_get_status",
    "lvt_amd_default_params", "lvt_amd_params_from_file", "lvt_amd_create", "lvt_amd_reset",
    "lvt_amd_track_rgbd", "lvt_amd_track_device", "lvt_amd_track_device_async", "lvt_amd_wait",
    "lvt_amd_set_stream", "lvt_amd_last_error", "lvt_amd_get_counts", "lvt_amd_get_features",
    "lvt_amd_get_matches", "lvt_amd_get_row_matches", "lvt_amd_get_map", "lvt_amd_get_staged", "lvt_amd_get_candidate_lists",
    "lvt_amd_get_pose", "lvt_amd_get_last_pose", "lvt_amd_get_predicted_pose", "lvt_amd_get_plane", "lvt_amd_pnp", "lvt_amd_pnp_detail",
    "lvt_amd_hamming_match_batched", "lvt_amd_hamming_match_batched_n", "lvt_amd_rectifier_create", "lvt_amd_rectifier_destroy",
    "lvt_amd_rectify_device", "lvt_amd_rectify", "lvt_amd_rectifier_get_maps", "lvt_amd_remap_device",
    "lvt_amd_rectifier_create_lens", "lvt_amd_rectifier_get_info",
    "lvt_amd_odometry_create", "lvt_amd_odometry_destroy", "lvt_amd_odometry_reset", "lvt_amd_odometry_push_pose", "lvt_amd_odometry_update", "lvt_amd_profile_enable", "lvt_amd_profile_read", "lvt_amd_get_debug", "lvt_amd_get_timeline", "lvt_amd_get_ordering",
    "lvt_amd_batch_create", "lvt_amd_batch_size", "lvt_amd_batch_track_device_async", "lvt_amd_batch_wait",
    "lvt_amd_batch_get_counts", "lvt_amd_create_on_device", "lvt_amd_get_device", "lvt_amd_wait_status", "lvt_amd_get_host_stats",
    "lvt_amd_track_async", "lvt_amd_track_rgbd_async", "lvt_amd_pnp_trace", "lvt_amd_create_pooled", "lvt_amd_wait_pose",
    "lvt_amd_batch_create_mixed", "lvt_amd_batch_track_device_async_mixed", "lvt_amd_batch_get_params", "lvt_amd_batch_mixed_tables",
    "lvt_amd_track_rgbd_device", "lvt_amd_track_rgbd_device_async", "lvt_amd_track_rgbd16", "lvt_amd_track_rgbd16_async",
    "lvt_amd_batch_track_rgbd_device_async",
    "lvt_amd_set_rectifiers", "lvt_amd_batch_set_rectifiers",
    "lvt_amd_set_pixel_format", "lvt_amd_batch_set_pixel_format", "lvt_amd_get_pixel_format",
    "lvt_amd_motion_predict",
    "lvt_amd_snapshot_take", "lvt_amd_snapshot_apply", "lvt_amd_batch_snapshot_take", "lvt_amd_batch_snapshot_apply", "lvt_amd_snapshot_get_info",
    "lvt_amd_snapshot_get_params", "lvt_amd_snapshot_export", "lvt_amd_snapshot_import", "lvt_amd_snapshot_describe", "lvt_amd_snapshot_destroy",
    "lvt_amd_batch_reset",
    "lvt_amd_enable_pose_info", "lvt_amd_get_pose_info", "lvt_amd_pose_info_eval", "lvt_amd_pose_info_to_ros",
    "lvt_amd_odometry_push_pose_cov", "lvt_amd_odometry_update_cov",
    "lvt_amd_set_depth_camera", "lvt_amd_batch_set_depth_camera", "lvt_amd_get_depth_camera", "lvt_amd_register_depth_device",
    "lvt_amd_set_equalisation", "lvt_amd_batch_set_equalisation", "lvt_amd_get_equalisation", "lvt_amd_equalise_device", "lvt_amd_equalisation_plan",
    "lvt_amd_set_sensor_format", "lvt_amd_batch_set_sensor_format", "lvt_amd_get_sensor_format", "lvt_amd_get_sensor_window", "lvt_amd_convert_sensor_device",
    "lvt_amd_set_reduction", "lvt_amd_batch_set_reduction", "lvt_amd_get_reduction", "lvt_amd_reduce_device", "lvt_amd_lens_reduced",
    "lvt_amd_set_mask", "lvt_amd_batch_set_mask", "lvt_amd_set_mask_device", "lvt_amd_batch_set_mask_device", "lvt_amd_get_mask_stats", "lvt_amd_mask_features",
    "lvt_amd_set_label_mask", "lvt_amd_batch_set_label_mask", "lvt_amd_get_label_mask", "lvt_amd_frame_labels", "lvt_amd_frame_labels_device", "lvt_amd_build_label_mask",
    "lvt_amd_depth_guard_default", "lvt_amd_set_depth_guard", "lvt_amd_batch_set_depth_guard", "lvt_amd_get_depth_guard", "lvt_amd_get_depth_guard_stats", "lvt_amd_depth_guard_features",
    "lvt_amd_relocalise", "lvt_amd_batch_relocalise", "lvt_amd_odometry_set_relocalisation", "lvt_amd_reloc_default_config", "lvt_amd_reloc_slice_length", "lvt_amd_reloc_match_device", "lvt_amd_reloc_solve", "lvt_amd_reloc_correspond",
]

N_COUNTS = 32
COUNT_NAMES = ["n_left", "n_right", "map_size", "staged_size", "n_matches", "second_pass", "n_row_matches",
               "n_triangulated", "triangulated", "retry_left", "retry_right", "pnp_iters", "pnp_inliers",
               "map_size_at_match", "n_staged_erased", "n_staged_promoted", "n_culled", "frame", "overflow", "pnp_borderline", "row_fallback", "pnp_trials", "pnp_rejections", "pnp_terminates"]

LISTS_WHICH = {"map": 0, "staged": 1, "row": 2}   # LVT_AMD_LISTS_*
LIST_INFO_NAMES = ["kc", "stood_down_map", "stood_down_row", "pass2", "n_early", "binned", "n"]   # lvt_amd_list_info

eState_NOT_INITIALIZED, eState_TRACKING, eState_LOST = 1, 2, 3
eSensor_STEREO, eSensor_RGBD = 1, 2
PIX_GRAY8, PIX_BGR8, PIX_RGB8, PIX_BGRA8, PIX_RGBA8 = 0, 1, 2, 3, 4   # LVT_AMD_PIX_*: interleaved 8-bit formats a handle / a batch sequence takes its frames in
PIX_BPP = {PIX_GRAY8: 1, PIX_BGR8: 3, PIX_RGB8: 3, PIX_BGRA8: 4, PIX_RGBA8: 4}
# LVT_AMD_SENSOR_*: the camera's own layouts a handle / a batch sequence takes its frames in (SensorFormat): 8-bit Bayer mosaics, YUV 4:2:2, 16-bit gray
SENSOR_NONE = 0
SENSOR_BAYER_RGGB8, SENSOR_BAYER_BGGR8, SENSOR_BAYER_GRBG8, SENSOR_BAYER_GBRG8 = 16, 17, 18, 19
SENSOR_YUYV, SENSOR_UYVY = 24, 25
SENSOR_MONO16 = 32
SENSOR_BPP = {SENSOR_NONE: 1, SENSOR_BAYER_RGGB8: 1, SENSOR_BAYER_BGGR8: 1, SENSOR_BAYER_GRBG8: 1, SENSOR_BAYER_GBRG8: 1, SENSOR_YUYV: 2, SENSOR_UYVY: 2, SENSOR_MONO16: 2}
DEPTH_F32, DEPTH_U16 = 0, 1   # LVT_AMD_DEPTH_F32 (metres) / LVT_AMD_DEPTH_U16 (raw sensor units: metres = raw * depth_scale)

_lib = None


def load_library():
    """dlopen the HIP library; raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C lvt_amd/csrc` "
                           "(there is no CPU fallback for the tracking path)")
    # PyTorch wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7, same as /opt/rocm's).  If this library
    # were loaded first, a later `import torch` would bring a SECOND HIP runtime into the process and whichever
    # initialises last reports "no ROCm-capable device".  Importing torch first makes the dynamic loader resolve our
    # DT_NEEDED libamdhip64.so.7 to the copy that is already mapped: one runtime per process.
    try:
        import torch  # noqa: F401
    except Exception:  # torch is optional: plain C / ctypes callers simply use the system runtime
        pass
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.lvt_create.restype = vp
    L.lvt_create.argtypes = [C.c_char_p, C.c_int]
    L.lvt_amd_create.restype = vp
    L.lvt_amd_create.argtypes = [vp, C.c_int]
    L.lvt_amd_create_on_device.restype = vp
    L.lvt_amd_create_on_device.argtypes = [vp, C.c_int, C.c_int]
    L.lvt_amd_get_device.argtypes = [vp]
    L.lvt_amd_create_pooled.restype = vp
    L.lvt_amd_create_pooled.argtypes = [vp, C.c_int, C.c_int]
    L.lvt_destroy.argtypes = [vp]
    L.lvt_amd_reset.argtypes = [vp]
    L.lvt_track.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.lvt_track_with_external_corners.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp]
    L.lvt_get_status.argtypes = [vp]
    L.lvt_amd_params_from_file.argtypes = [C.c_char_p, vp]
    L.lvt_amd_default_params.argtypes = [vp]
    L.lvt_amd_track_rgbd.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.lvt_amd_track_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.lvt_amd_track_device_async.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int]
    L.lvt_amd_wait.argtypes = [vp, vp, vp]
    L.lvt_amd_track_async.argtypes = [vp, vp, vp, C.c_int, C.c_int]
    L.lvt_amd_track_async.restype = C.c_int
    L.lvt_amd_track_rgbd_async.argtypes = [vp, vp, vp, C.c_int, C.c_int]
    L.lvt_amd_track_rgbd_async.restype = C.c_int
    L.lvt_amd_wait_status.argtypes = [vp, vp, vp]
    L.lvt_amd_wait_status.restype = C.c_int
    L.lvt_amd_set_stream.argtypes = [vp, vp]
    L.lvt_amd_last_error.restype = C.c_char_p
    L.lvt_amd_last_error.argtypes = [vp]
    L.lvt_amd_get_counts.argtypes = [vp, vp]
    L.lvt_amd_get_features.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int]
    L.lvt_amd_get_matches.argtypes = [vp, vp, vp, C.c_int]
    L.lvt_amd_get_row_matches.argtypes = [vp, vp, C.c_int]
    L.lvt_amd_get_map.argtypes = [vp, vp, vp, vp, vp, C.c_int]
    L.lvt_amd_get_staged.argtypes = [vp, vp, vp, vp, C.c_int]
    L.lvt_amd_get_candidate_lists.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    L.lvt_amd_get_candidate_lists.restype = C.c_int
    L.lvt_amd_get_pose.argtypes = [vp, vp, vp]
    L.lvt_amd_get_last_pose.argtypes = [vp, vp, vp]
    L.lvt_amd_get_predicted_pose.argtypes = [vp, vp, vp]
    L.lvt_amd_get_plane.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp]
    L.lvt_amd_pnp.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp]
    L.lvt_amd_pnp_detail.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.lvt_amd_pnp_trace.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]
    L.lvt_amd_motion_predict.argtypes = [vp, vp, vp, vp, vp]
    L.lvt_amd_motion_predict.restype = C.c_int
    L.lvt_amd_hamming_match_batched.restype = C.c_float
    L.lvt_amd_hamming_match_batched.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, vp, vp]
    L.lvt_amd_get_timeline.argtypes = [vp, vp]
    L.lvt_amd_get_ordering.argtypes = [vp]
    L.lvt_amd_get_ordering.restype = C.c_int
    L.lvt_amd_rectifier_create.restype = vp
    L.lvt_amd_rectifier_create.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int]
    L.lvt_amd_rectifier_destroy.argtypes = [vp]
    L.lvt_amd_rectify_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp]
    L.lvt_amd_rectify.argtypes = [vp, vp, vp]
    L.lvt_amd_rectifier_get_maps.argtypes = [vp, vp, vp]
    if hasattr(L, "lvt_amd_rectifier_create_lens"):   # (lens models: a library built before they existed -- LVT_AMD_LIB, A/B runs -- lacks them)
        L.lvt_amd_rectifier_create_lens.restype = vp
        L.lvt_amd_rectifier_create_lens.argtypes = [vp, vp, vp, C.c_int, C.c_int]
        L.lvt_amd_rectifier_get_info.argtypes = [vp, vp, vp]
    L.lvt_amd_remap_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]
    L.lvt_amd_remap_device.restype = C.c_int
    L.lvt_amd_odometry_create.restype = vp
    L.lvt_amd_odometry_create.argtypes = [vp, vp, C.c_int]
    L.lvt_amd_odometry_destroy.argtypes = [vp]
    L.lvt_amd_odometry_reset.argtypes = [vp]
    L.lvt_amd_odometry_push_pose.restype = C.c_int
    L.lvt_amd_odometry_push_pose.argtypes = [vp, vp, vp, C.c_int, C.c_double, vp, vp]
    L.lvt_amd_odometry_update.restype = C.c_int
    L.lvt_amd_odometry_update.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_double, vp, vp]
    L.lvt_amd_hamming_match_batched_n.restype = C.c_float
    L.lvt_amd_hamming_match_batched_n.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int]
    L.lvt_amd_profile_enable.argtypes = [vp, C.c_int]
    L.lvt_amd_batch_create.restype = vp
    L.lvt_amd_batch_create.argtypes = [vp, C.c_int, C.c_int]
    L.lvt_amd_batch_size.argtypes = [vp]
    L.lvt_amd_batch_track_device_async.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int]
    L.lvt_amd_batch_wait.argtypes = [vp, vp, vp, vp]
    L.lvt_amd_batch_get_counts.argtypes = [vp, C.c_int, vp]
    L.lvt_amd_batch_create_mixed.restype = vp
    L.lvt_amd_batch_create_mixed.argtypes = [vp, C.c_int, C.c_int]
    L.lvt_amd_batch_track_device_async_mixed.restype = C.c_int
    L.lvt_amd_batch_track_device_async_mixed.argtypes = [vp, vp, vp, vp, vp, vp]
    L.lvt_amd_batch_get_params.restype = C.c_int
    L.lvt_amd_batch_get_params.argtypes = [vp, C.c_int, vp]
    L.lvt_amd_batch_mixed_tables.restype = C.c_int
    L.lvt_amd_batch_mixed_tables.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, vp]
    L.lvt_amd_batch_size.restype = C.c_int
    # RGB-D on device planes / with 16-bit depth / in lock-step batches (a library built before they existed -- LVT_AMD_LIB, kernel A/B runs -- simply lacks them)
    for name, argtypes in (
            ("lvt_amd_track_rgbd_device_async", [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int]),
            ("lvt_amd_track_rgbd_device", [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, vp, vp]),
            ("lvt_amd_track_rgbd16", [vp, vp, vp, C.c_float, C.c_int, C.c_int, vp, vp]),
            ("lvt_amd_track_rgbd16_async", [vp, vp, vp, C.c_float, C.c_int, C.c_int]),
            ("lvt_amd_batch_track_rgbd_device_async", [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_float])):
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
    for name, argtypes in (("lvt_amd_set_rectifiers", [vp, vp, vp]), ("lvt_amd_batch_set_rectifiers", [vp, C.c_int, vp, vp])):   # (raw frames: likewise)
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
    for name, argtypes in (("lvt_amd_set_pixel_format", [vp, C.c_int]), ("lvt_amd_batch_set_pixel_format", [vp, C.c_int, C.c_int]),
                           ("lvt_amd_get_pixel_format", [vp, C.c_int])):   # (colour frames: likewise)
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
    for name, argtypes, restype in (   # (snapshots: likewise)
            ("lvt_amd_snapshot_take", [vp, C.c_int], vp), ("lvt_amd_snapshot_apply", [vp, C.c_int, vp], C.c_int),
            ("lvt_amd_batch_snapshot_take", [vp, vp], C.c_int), ("lvt_amd_batch_snapshot_apply", [vp, vp], C.c_int),
            ("lvt_amd_snapshot_get_info", [vp, vp], C.c_int), ("lvt_amd_snapshot_get_params", [vp, vp], C.c_int),
            ("lvt_amd_snapshot_export", [vp, vp, C.c_longlong], C.c_longlong), ("lvt_amd_snapshot_import", [vp, C.c_longlong, C.c_int], vp),
            ("lvt_amd_snapshot_describe", [vp, C.c_longlong, vp, vp], C.c_int), ("lvt_amd_snapshot_destroy", [vp], None),
            ("lvt_amd_batch_reset", [vp, C.c_int], C.c_int)):
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, restype
    for name, argtypes, restype in (   # (pose uncertainty: likewise)
            ("lvt_amd_enable_pose_info", [vp, C.c_int], C.c_int), ("lvt_amd_get_pose_info", [vp, C.c_int, vp], C.c_int),
            ("lvt_amd_pose_info_eval", [vp, vp, vp, vp, vp, C.c_int, vp], C.c_int), ("lvt_amd_pose_info_to_ros", [vp, vp, vp], None),
            ("lvt_amd_odometry_push_pose_cov", [vp, vp, vp, C.c_int, C.c_double, vp, vp, vp, vp], C.c_int),
            ("lvt_amd_odometry_update_cov", [vp, vp, vp, C.c_int, C.c_int, C.c_double, vp, vp, vp], C.c_int)):
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, restype
    for name, argtypes in (   # (unregistered depth: likewise)
            ("lvt_amd_set_depth_camera", [vp, vp]), ("lvt_amd_batch_set_depth_camera", [vp, C.c_int, vp]), ("lvt_amd_get_depth_camera", [vp, C.c_int, vp]),
            ("lvt_amd_register_depth_device", [vp, vp, vp, C.c_int, C.c_int, C.c_float, vp, C.c_int, vp])):
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
    for name, argtypes in (   # (dim frames: likewise)
            ("lvt_amd_set_equalisation", [vp, vp]), ("lvt_amd_batch_set_equalisation", [vp, C.c_int, vp]), ("lvt_amd_get_equalisation", [vp, C.c_int, vp]),
            ("lvt_amd_equalise_device", [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]), ("lvt_amd_equalisation_plan", [vp, C.c_int, C.c_int, vp, vp])):
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
    for name, argtypes in (   # (sensor formats: likewise)
            ("lvt_amd_set_sensor_format", [vp, vp]), ("lvt_amd_batch_set_sensor_format", [vp, C.c_int, vp]), ("lvt_amd_get_sensor_format", [vp, C.c_int, vp]),
            ("lvt_amd_get_sensor_window", [vp, C.c_int, C.c_int, vp, vp]),
            ("lvt_amd_convert_sensor_device", [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp])):
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
    for name, argtypes in (   # (frame reduction: likewise)
            ("lvt_amd_set_reduction", [vp, vp]), ("lvt_amd_batch_set_reduction", [vp, C.c_int, vp]), ("lvt_amd_get_reduction", [vp, C.c_int, vp]),
            ("lvt_amd_reduce_device", [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]), ("lvt_amd_lens_reduced", [vp, C.c_int, vp])):
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
    for name, argtypes in (   # (feature masks: likewise)
            ("lvt_amd_set_mask", [vp, vp, vp]), ("lvt_amd_batch_set_mask", [vp, C.c_int, vp, vp]), ("lvt_amd_set_mask_device", [vp, vp, C.c_int, vp, C.c_int]),
            ("lvt_amd_batch_set_mask_device", [vp, C.c_int, vp, C.c_int, vp, C.c_int]), ("lvt_amd_get_mask_stats", [vp, C.c_int, vp]),
            ("lvt_amd_mask_features", [C.c_int] + [vp] * 9 + [C.c_int] * 3)):
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
    for name, argtypes in (   # (label masks: likewise)
            ("lvt_amd_set_label_mask", [vp, vp]), ("lvt_amd_batch_set_label_mask", [vp, C.c_int, vp]), ("lvt_amd_get_label_mask", [vp, C.c_int, vp]),
            ("lvt_amd_frame_labels", [vp, C.c_int, vp, vp]), ("lvt_amd_frame_labels_device", [vp, C.c_int, vp, C.c_int, vp, C.c_int]),
            ("lvt_amd_build_label_mask", [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int])):
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
    for name, argtypes, restype in (   # (depth guard: likewise)
            ("lvt_amd_depth_guard_default", [vp], None), ("lvt_amd_set_depth_guard", [vp, vp], C.c_int), ("lvt_amd_batch_set_depth_guard", [vp, C.c_int, vp], C.c_int),
            ("lvt_amd_get_depth_guard", [vp, C.c_int, vp], C.c_int), ("lvt_amd_get_depth_guard_stats", [vp, C.c_int, vp], C.c_int),
            ("lvt_amd_depth_guard_features", [C.c_int] + [vp] * 9 + [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, vp], C.c_int)):
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, restype
    for name, argtypes, restype in (   # (relocalisation: likewise)
            ("lvt_amd_relocalise", [vp, vp, vp], C.c_int), ("lvt_amd_batch_relocalise", [vp, C.c_int, vp, vp], C.c_int),
            ("lvt_amd_odometry_set_relocalisation", [vp, vp, C.c_int], C.c_int), ("lvt_amd_reloc_default_config", [vp], None), ("lvt_amd_reloc_slice_length", [C.c_int], C.c_int),
            ("lvt_amd_reloc_match_device", [vp, C.c_int, vp, C.c_int, vp, vp], C.c_float),
            ("lvt_amd_reloc_solve", [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp], C.c_int),
            ("lvt_amd_reloc_correspond", [vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int] + [vp] * 8, C.c_int)):
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, restype
    L.lvt_amd_get_debug.argtypes = [vp, vp]
    L.lvt_amd_get_host_stats.argtypes = [vp, vp]
    L.lvt_amd_profile_read.argtypes = [vp, C.c_int, C.c_char_p, C.c_int, vp, vp]
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _u8(img, bpp=1):
    """a contiguous uint8 image of bpp bytes per pixel: (H, W) for gray, (H, W, bpp) for a colour format -- anything else raises"""
    a = img if (isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.flags.c_contiguous) else np.ascontiguousarray(img, dtype=np.uint8)
    if bpp == 1:
        assert a.ndim == 2
    elif a.ndim != 3 or a.shape[2] != bpp:
        raise ValueError(f"an image of shape {a.shape} on a handle whose pixel format has {bpp} bytes per pixel: expected (H, W, {bpp})")
    return a


def _record_of(fn_name, Struct, handle, seq):
    """a per-sequence property record through its getter: the record, None where the sequence has none"""
    r = Struct()
    rc = getattr(load_library(), fn_name)(handle, int(seq), C.byref(r))
    if rc < 0:
        raise IndexError(f"{fn_name}: bad handle or no sequence {seq}")
    return r if rc == 1 else None


def _stats_of(fn_name, width, handle, seq):
    """a filter's `width` stats words of the last collected frame as ints, None where the getter has nothing to report"""
    out = np.zeros(width, dtype=np.int32)
    rc = getattr(load_library(), fn_name)(handle, int(seq), _p(out))
    if rc < 0:
        raise IndexError(f"{fn_name}: bad handle or no sequence {seq}")
    return [int(v) for v in out] if rc == 1 else None


def _feature_arrays(x, y, resp, bx, by, depth, hcx, hcy):
    """the eight arrays of n features as a filter's stage entry takes them, as fresh copies: (n, [six float32, two int16])"""
    a = [np.array(v, dtype=np.float32).ravel() for v in (x, y, resp, bx, by, depth)] + [np.array(v, dtype=np.int16).ravel() for v in (hcx, hcy)]
    if any(v.size != a[0].size for v in a):
        raise ValueError("the eight feature arrays differ in length")
    return a[0].size, a


def _padded_plane(a, dtypes, width=None, height=None):
    """a 2-D array of one of `dtypes` whose row stride is the pitch (a view into a wider array keeps its pitch), as the plane lies in memory: (the rows with
    their padding as one flat copy, pitch in elements, width, height), the last two defaulting to the array's shape.  None for any other array"""
    a = np.asarray(a)
    if a.dtype not in dtypes or a.ndim != 2 or a.strides[1] != a.itemsize or a.strides[0] < a.shape[1] * a.itemsize or a.strides[0] % a.itemsize:
        return None
    height = a.shape[0] if height is None else int(height)
    pitch = a.strides[0] // a.itemsize
    flat = np.zeros(pitch * height, dtype=a.dtype)
    np.lib.stride_tricks.as_strided(flat, shape=(height, a.shape[1]), strides=a.strides)[:] = a[:height]
    return flat, pitch, a.shape[1] if width is None else int(width), height


class DepthCamera(C.Structure):
    """lvt_amd_depth_camera: the camera an RGB-D sensor delivers its depth plane in (include/lvt_amd_ext.h, UNREGISTERED DEPTH) -- its image size, its pinhole
    (no distortion) and p_colour = R p_depth + t in metres"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("_R", C.c_float * 9), ("_t", C.c_float * 3)]

    def __init__(self, width=0, height=0, fx=0.0, fy=0.0, cx=0.0, cy=0.0, R=None, t=None):
        super().__init__(int(width), int(height), float(fx), float(fy), float(cx), float(cy))
        self.R = np.eye(3) if R is None else R
        self.t = np.zeros(3) if t is None else t

    @property
    def R(self) -> np.ndarray:
        return np.array(self._R, dtype=np.float32).reshape(3, 3)

    @R.setter
    def R(self, v):
        self._R = (C.c_float * 9)(*[float(x) for x in np.asarray(v, dtype=np.float64).reshape(9)])

    @property
    def t(self) -> np.ndarray:
        return np.array(self._t, dtype=np.float32)

    @t.setter
    def t(self, v):
        self._t = (C.c_float * 3)(*[float(x) for x in np.asarray(v, dtype=np.float64).reshape(3)])

    def to_bytes(self) -> bytes:
        return bytes(memoryview(self))


def _depth_camera_of(handle, seq):
    return _record_of("lvt_amd_get_depth_camera", DepthCamera, handle, seq)


def register_depth_device(cam: DepthCamera, params: LvtParameters, d_depth: int, depth_pitch: int, depth_format: int, depth_scale: float, d_out: int,
                          out_pitch: int, stream: int = 0) -> int:
    """stage entry: the depth registration alone on device planes (pitches in bytes; d_out fp32, out_pitch / 4 >= img_width words per row, img_height rows, every
    word written); 0 / -1"""
    pod = params.to_pod()
    return load_library().lvt_amd_register_depth_device(C.byref(cam), C.byref(pod), C.c_void_p(d_depth), int(depth_pitch), int(depth_format), float(depth_scale),
                                                        C.c_void_p(d_out), int(out_pitch), C.c_void_p(stream))


class Equalisation(C.Structure):
    """lvt_amd_equalisation: CLAHE contrast equalisation of the gray plane the detector reads (include/lvt_amd_ext.h, DIM frames) -- tiles = (tiles_x, tiles_y),
    1 ... 16 each and no more than the image's width / height; clip_limit finite and > 0"""
    _fields_ = [("tiles_x", C.c_int), ("tiles_y", C.c_int), ("clip_limit", C.c_float)]

    def __init__(self, tiles=(8, 8), clip_limit=3.0):
        super().__init__(int(tiles[0]), int(tiles[1]), float(clip_limit))

    @property
    def tiles(self):
        return (int(self.tiles_x), int(self.tiles_y))

    def __repr__(self):
        return f"Equalisation(tiles={self.tiles}, clip_limit={float(self.clip_limit)!r})"


def _equalisation_of(handle, seq):
    return _record_of("lvt_amd_get_equalisation", Equalisation, handle, seq)


def equalise_device(cfg: Equalisation, d_src: int, src_pitch: int, width: int, height: int, d_dst: int, dst_pitch: int, stream: int = 0) -> int:
    """stage entry: the equalisation alone on device planes (u8; d_src any address, src_pitch >= width; d_dst 4-byte aligned, dst_pitch % 4 == 0 and >= width:
    every byte of height x dst_pitch is written, the columns from width on as zero); 0 / -1"""
    return load_library().lvt_amd_equalise_device(C.byref(cfg), C.c_void_p(d_src), int(src_pitch), int(width), int(height), C.c_void_p(d_dst), int(dst_pitch),
                                                  C.c_void_p(stream))


def equalisation_plan(cfg: Equalisation, width: int, height: int):
    """steps 1 and 2 of the definition for a width x height image: {Wp, Hp, tile_w, tile_h, area, clip, lut_scale}; None for a record the setter would refuse.
    Host code: needs the library, not a GPU"""
    out = (C.c_int * 6)()
    scale = C.c_float(0)
    if load_library().lvt_amd_equalisation_plan(C.byref(cfg), int(width), int(height), out, C.byref(scale)) != 0:
        return None
    d = dict(zip(("Wp", "Hp", "tile_w", "tile_h", "area", "clip"), (int(x) for x in out)))
    d["lut_scale"] = np.float32(scale.value)
    return d


class SensorFormat(C.Structure):
    """lvt_amd_sensor_format: the camera's own pixel layout, turned into 8-bit gray at the head of the feature stage (include/lvt_amd_ext.h, SENSOR FORMATS) --
    format SENSOR_NONE = off, a Bayer pattern, SENSOR_YUYV / SENSOR_UYVY, or SENSOR_MONO16 with a window: fixed [lo, hi] (auto_window = 0) or found per
    frame from the frame's histogram (auto_window = 1: lo_permille / hi_permille of the pixels may fall below / above it, min_span is its smallest width)"""
    _fields_ = [("format", C.c_int), ("auto_window", C.c_int), ("lo", C.c_int), ("hi", C.c_int), ("lo_permille", C.c_int), ("hi_permille", C.c_int),
                ("min_span", C.c_int), ("reserved", C.c_int * 1)]

    def __init__(self, format=SENSOR_NONE, auto_window=0, lo=0, hi=65535, lo_permille=0, hi_permille=0, min_span=1):
        super().__init__(int(format), int(auto_window), int(lo), int(hi), int(lo_permille), int(hi_permille), int(min_span))

    def __repr__(self):
        return (f"SensorFormat(format={int(self.format)}, auto_window={int(self.auto_window)}, lo={int(self.lo)}, hi={int(self.hi)}, "
                f"lo_permille={int(self.lo_permille)}, hi_permille={int(self.hi_permille)}, min_span={int(self.min_span)})")


def _sensor_format_of(handle, seq):
    return _record_of("lvt_amd_get_sensor_format", SensorFormat, handle, seq)


def _sensor_format_arg(cfg, kw):
    if cfg is None:
        cfg = SensorFormat(**kw) if kw else SensorFormat(SENSOR_NONE)   # (None: off)
    elif not isinstance(cfg, SensorFormat):
        cfg = SensorFormat(int(cfg), **kw)                               # (a bare format constant)
    return cfg


def _sensor_window_of(handle, seq, eye):
    lo, hi = C.c_int(0), C.c_int(0)
    rc = load_library().lvt_amd_get_sensor_window(handle, int(seq), int(eye), C.byref(lo), C.byref(hi))
    if rc < 0:
        raise IndexError(f"lvt_amd_get_sensor_window: bad handle, no sequence {seq} or no image {eye}")
    return (lo.value, hi.value) if rc == 1 else None


def sensor_plane(img, fmt: int):
    """a sensor's host plane as bytes, (H, W) for a Bayer mosaic and (H, W, 2) for the 16-bit-per-pixel formats: a YUV 4:2:2 plane may come as (H, 2 W) or
    (H, W, 2) uint8, a MONO16 plane is (H, W) uint16 (little-endian, as this host stores it).  Views, no copies, where the array is contiguous."""
    fmt = int(fmt)
    if fmt == SENSOR_MONO16:
        a = img if (isinstance(img, np.ndarray) and img.dtype == np.uint16 and img.flags.c_contiguous) else np.ascontiguousarray(img, dtype=np.uint16)
        if a.ndim != 2:
            raise ValueError(f"a MONO16 plane of shape {a.shape}: expected (H, W) uint16")
        return a.view(np.uint8).reshape(a.shape[0], a.shape[1], 2)
    a = img if (isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.flags.c_contiguous) else np.ascontiguousarray(img, dtype=np.uint8)
    if fmt in (SENSOR_YUYV, SENSOR_UYVY) and a.ndim == 2:
        if a.shape[1] % 2:
            raise ValueError(f"a YUV 4:2:2 plane of shape {a.shape}: a row is 2 W bytes")
        return a.reshape(a.shape[0], a.shape[1] // 2, 2)
    return a


def convert_sensor_device(cfg: SensorFormat, d_src: int, src_pitch: int, width: int, height: int, d_dst: int, dst_pitch: int):
    """stage entry: the sensor-format conversion alone on device planes (d_src: `height` rows of src_pitch bytes, any address -- MONO16: even --; d_dst
    4-byte aligned, dst_pitch % 4 == 0 and >= width: every byte of height x dst_pitch is written, the padding columns as zero).  Returns (rc, window):
    (0, (lo, hi)) for MONO16, (0, None) otherwise, (-1, None) on a refusal, whose sentence is last_call_error()."""
    win = (C.c_int * 2)(0, 0)
    rc = load_library().lvt_amd_convert_sensor_device(C.byref(cfg) if cfg is not None else None, C.c_void_p(d_src), int(src_pitch), int(width), int(height),
                                                      C.c_void_p(d_dst), int(dst_pitch), win)
    return rc, ((win[0], win[1]) if rc == 0 and int(cfg.format) == SENSOR_MONO16 else None)


class Reduction(C.Structure):
    """lvt_amd_reduction: large frames averaged down by an integer factor at the head of the feature stage (include/lvt_amd_ext.h, FRAME REDUCTION) -- factor
    1 = off, 2 ... 8; width x height is the FRAME's size, as every entry point then takes it: width // factor x height // factor must be the sequence's base
    size (its rectifiers' source size, else its own image size)"""
    _fields_ = [("factor", C.c_int), ("width", C.c_int), ("height", C.c_int)]

    def __init__(self, factor=1, width=1, height=1):
        super().__init__(int(factor), int(width), int(height))

    def __repr__(self):
        return f"Reduction(factor={int(self.factor)}, width={int(self.width)}, height={int(self.height)})"


def _reduction_of(handle, seq):
    return _record_of("lvt_amd_get_reduction", Reduction, handle, seq)


def _reduction_arg(cfg, kw):
    if cfg is None:
        cfg = Reduction(**kw) if kw else Reduction(1, 1, 1)   # (None: off)
    return cfg


def reduce_device(d_src: int, src_w: int, src_h: int, src_pitch: int, factor: int, d_dst: int, dst_pitch: int):
    """stage entry: the reduction alone on device planes (u8; d_src any address, src_pitch >= src_w; d_dst 4-byte aligned, dst_pitch % 4 == 0 and
    >= src_w // factor: every byte of src_h // factor rows x dst_pitch is written, the padding columns as zero).  Returns (rc, kernels launched): (0, 1), or
    (-1, 0) on a refusal, whose sentence is last_call_error()."""
    n = C.c_int(-1)
    rc = load_library().lvt_amd_reduce_device(C.c_void_p(d_src), int(src_w), int(src_h), int(src_pitch), int(factor), C.c_void_p(d_dst), int(dst_pitch), C.byref(n))
    return rc, n.value


def reduced_intrinsics(fx: float, fy: float, cx: float, cy: float, f: int):
    """(fx, fy, cx, cy) of the image reduced by f: reduced pixel x covers source columns [f x, f x + f), so fx' = fx / f and cx' = (cx + 0.5) / f - 0.5"""
    f = float(f)
    return fx / f, fy / f, (cx + 0.5) / f - 0.5, (cy + 0.5) / f - 0.5


def _mask_of(handle, seq, mask):
    """a feature mask as the C-ABI takes it: a contiguous (H, W) uint8 array of the sequence's image size (bool arrays become 0 / 1), or None.  The C-ABI has
    no size argument for a host mask: an array of another shape would be read past its end, so it raises here"""
    if mask is None:
        return None
    a = np.ascontiguousarray(mask, dtype=np.uint8)
    pod = ParamsPOD()
    if load_library().lvt_amd_batch_get_params(handle, int(seq), C.byref(pod)) and a.shape != (pod.img_height, pod.img_width):
        raise ValueError(f"a mask of shape {a.shape} on a sequence of {pod.img_height} x {pod.img_width} pixels")
    if a.ndim != 2:
        raise ValueError(f"a mask of shape {a.shape}: expected (H, W)")
    return a


def _mask_stats_of(handle, seq):
    out = _stats_of("lvt_amd_get_mask_stats", 4, handle, seq)
    return out and {"kept": (out[0], out[2]), "dropped": (out[1], out[3])}


def mask_features(x, y, resp, bx, by, depth, hcx, hcy, mask, width: int = None, height: int = None):
    """stage entry: the feature-mask kernel alone on n <= 4096 features (include/lvt_amd_ext.h, FEATURE MASKS).  mask: a 2-D uint8 array whose row stride is the
    pitch (a view into a wider array keeps its pitch); width / height default to its shape.  Returns (n_kept, x, y, resp, bx, by, depth, hcx, hcy): the arrays as
    the kernel left them, the first n_kept elements being the kept features in order.  RuntimeError with the reason when refused."""
    n, arrays = _feature_arrays(x, y, resp, bx, by, depth, hcx, hcy)
    plane = _padded_plane(mask, (np.uint8,), width, height)
    if plane is None:
        raise ValueError("mask: a 2-D uint8 array with contiguous rows")
    flat, pitch, width, height = plane
    rc = load_library().lvt_amd_mask_features(n, *[_p(a) for a in arrays], _p(flat), width, height, pitch)
    if rc < 0:
        raise RuntimeError((load_library().lvt_amd_last_error(None) or b"").decode() or "lvt_amd_mask_features failed")
    return (rc, *arrays)


class LabelMask(C.Structure):
    """lvt_amd_label_mask: how the label image that travels with a frame becomes that frame's feature mask (include/lvt_amd_ext.h, LABEL MASKS) -- the label
    image's size (label_width, label_height, 1 ... 8192 each, independent of the image size), the labels that forbid key points (`drop`: an iterable of
    label values, or 256 flags) and `dilate` (0 ... 15 pixels of the detector's grid)"""
    _fields_ = [("label_width", C.c_int), ("label_height", C.c_int), ("drop", C.c_uint8 * 256), ("dilate", C.c_int)]

    def __init__(self, label_width=0, label_height=0, drop=(), dilate=0):
        flags = (C.c_uint8 * 256)()
        drop = list(drop)
        if len(drop) == 256:
            for l, v in enumerate(drop):
                flags[l] = 1 if v else 0
        else:
            for l in drop:
                flags[int(l)] = 1
        super().__init__(int(label_width), int(label_height), flags, int(dilate))

    def dropped(self):
        """the label values that forbid key points"""
        return [l for l in range(256) if self.drop[l]]

    def __repr__(self):
        return f"LabelMask(label_width={int(self.label_width)}, label_height={int(self.label_height)}, drop={self.dropped()}, dilate={int(self.dilate)})"


def _labels_of(handle, seq, labels):
    """a label image as lvt_amd_frame_labels takes it: a contiguous (label_height, label_width) uint8 array, or None.  The C-ABI has no size argument for a
    host image: an array of another shape would be read past its end, so it raises here"""
    if labels is None:
        return None
    a = np.ascontiguousarray(labels, dtype=np.uint8)
    rec = _record_of("lvt_amd_get_label_mask", LabelMask, handle, seq)
    if rec is not None and a.shape != (rec.label_height, rec.label_width):
        raise ValueError(f"a label image of shape {a.shape} under a record of {rec.label_height} x {rec.label_width} labels")
    return a


def _frame_labels(handle, seq, left, right, pitch_left, pitch_right):
    """numpy arrays (host images), or device addresses with their pitches"""
    L = load_library()
    if isinstance(left, (int, np.integer)) or isinstance(right, (int, np.integer)):
        return L.lvt_amd_frame_labels_device(handle, int(seq), C.c_void_p(int(left) if left else None), int(pitch_left), C.c_void_p(int(right) if right else None),
                                             int(pitch_right))
    l, r = _labels_of(handle, seq, left), _labels_of(handle, seq, right)
    return L.lvt_amd_frame_labels(handle, int(seq), _p(l), _p(r))


def build_label_mask(cfg: LabelMask, labels, width: int, height: int, static=None, out_pitch: int = None):
    """stage entry: k_label_mask alone (include/lvt_amd_ext.h, LABEL MASKS).  labels: a 2-D uint8 array of cfg's size whose row stride is the pitch and whose
    address is kept modulo 4 on the device (a view keeps both); static: None or a 2-D uint8 array of (height, width), likewise.  Returns the (height,
    out_pitch) uint8 plane, the padding columns included (out_pitch defaults to the width rounded up to 64).  RuntimeError with the reason when refused."""
    def view(a, what):
        a = np.asarray(a)
        if a.dtype != np.uint8 or a.ndim != 2 or a.strides[1] != 1 or a.strides[0] < a.shape[1]:
            raise ValueError(f"{what}: a 2-D uint8 array with contiguous rows")
        return a
    labels = view(labels, "labels")
    if labels.shape != (cfg.label_height, cfg.label_width):
        raise ValueError(f"labels of shape {labels.shape} under a record of {cfg.label_height} x {cfg.label_width} labels")
    if static is not None:
        static = view(static, "static")
        if static.shape != (height, width):
            raise ValueError(f"a static mask of shape {static.shape} on an image of {height} x {width} pixels")
    out_pitch = (int(width) + 63) // 64 * 64 if out_pitch is None else int(out_pitch)
    out = np.full((int(height), max(out_pitch, 1)), 0xEE, np.uint8)
    rc = load_library().lvt_amd_build_label_mask(C.byref(cfg), C.c_void_p(labels.ctypes.data), int(labels.strides[0]), int(width), int(height),
                                                 C.c_void_p(static.ctypes.data) if static is not None else None, int(static.strides[0]) if static is not None else 0,
                                                 _p(out), out_pitch)
    if rc != 0:
        raise RuntimeError((load_library().lvt_amd_last_error(None) or b"").decode() or "lvt_amd_build_label_mask failed")
    return out


class DepthGuard(C.Structure):
    """lvt_amd_depth_guard: an RGB-D key point is kept when at least min_support of the (2 * radius + 1)^2 - 1 depth samples around its own are valid and within
    tol_abs + tol_rel * depth of it (include/lvt_amd_ext.h, DEPTH GUARD) -- radius 1 ... 3, min_support 1 ... (2 * radius + 1)^2 - 1, tolerances finite and >= 0.
    The defaults are lvt_amd_depth_guard_default's"""
    _fields_ = [("radius", C.c_int), ("min_support", C.c_int), ("tol_abs", C.c_float), ("tol_rel", C.c_float)]

    def __init__(self, radius=1, min_support=4, tol_abs=0.01, tol_rel=0.02):
        super().__init__(int(radius), int(min_support), float(tol_abs), float(tol_rel))

    def __repr__(self):
        return f"DepthGuard(radius={int(self.radius)}, min_support={int(self.min_support)}, tol_abs={float(self.tol_abs)!r}, tol_rel={float(self.tol_rel)!r})"


def depth_guard_default() -> DepthGuard:
    """the record lvt_amd_depth_guard_default fills"""
    g = DepthGuard(0, 0, 0.0, 0.0)
    load_library().lvt_amd_depth_guard_default(C.byref(g))
    return g


def _depth_guard_arg(cfg, kw):
    if cfg is None and kw:
        cfg = DepthGuard(**kw)
    return cfg


def _depth_guard_of(handle, seq):
    return _record_of("lvt_amd_get_depth_guard", DepthGuard, handle, seq)


def _depth_guard_stats_of(handle, seq):
    out = _stats_of("lvt_amd_get_depth_guard_stats", 2, handle, seq)
    return out and {"kept": out[0], "dropped": out[1]}


def depth_guard_features(x, y, resp, bx, by, depth_of, hcx, hcy, depth, cfg: DepthGuard, near_plane: float, far_plane: float, depth_scale: float = 0.0,
                         width: int = None, height: int = None):
    """stage entry: the depth-guard kernel alone on n <= 4096 features (include/lvt_amd_ext.h, DEPTH GUARD).  depth: a 2-D float32 (metres) or uint16 (raw units,
    metres = raw * depth_scale) array whose row stride is the pitch (a view into a wider array keeps its pitch); width / height default to its shape.  Returns
    (n_kept, x, y, resp, bx, by, depth_of, hcx, hcy): the arrays as the kernel left them, the first n_kept elements being the kept features in order.
    RuntimeError with the reason when refused."""
    n, arrays = _feature_arrays(x, y, resp, bx, by, depth_of, hcx, hcy)
    plane = _padded_plane(depth, (np.float32, np.uint16), width, height)
    if plane is None:
        raise ValueError("depth: a 2-D float32 or uint16 array with contiguous rows")
    flat, pitch, width, height = plane
    rc = load_library().lvt_amd_depth_guard_features(n, *[_p(a) for a in arrays], _p(flat), 1 if flat.dtype == np.uint16 else 0, float(depth_scale), width, height,
                                                     pitch, float(near_plane), float(far_plane), C.byref(cfg))
    if rc < 0:
        raise RuntimeError((load_library().lvt_amd_last_error(None) or b"").decode() or "lvt_amd_depth_guard_features failed")
    return (rc, *arrays)


class SnapshotInfo(C.Structure):
    """lvt_amd_snapshot_info"""
    _fields_ = [(n, C.c_int) for n in ("version", "sensor_type", "state", "frame_number", "map_n", "staged_n", "src_map_cur", "src_staged_cur", "device")] + \
               [("bytes", C.c_longlong)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


POSE_INFO_NONE, POSE_INFO_VALID, POSE_INFO_DEGENERATE = 0, 1, 2
POSE_INFO_SIZE = 616   # sizeof(lvt_amd_pose_info), LVT_AMD_POSE_INFO_SIZE: pinned in the header too


class PoseInfo(C.Structure):
    """lvt_amd_pose_info: the information matrix of a frame's 2D-3D edges at the published pose and its inverse (include/lvt_amd_ext.h, POSE UNCERTAINTY).
    Perturbation (dp on world axes, dtheta on camera axes), order px py pz thetax thetay thetaz, unit pixel noise."""
    _fields_ = [("_cov", C.c_double * 36), ("_info", C.c_double * 36), ("chi2", C.c_double), ("sq_err", C.c_double),
                ("n_edges", C.c_int), ("n_inliers", C.c_int), ("n_borderline", C.c_int), ("status", C.c_int), ("frame", C.c_int), ("reserved", C.c_int)]

    @property
    def cov(self) -> np.ndarray:
        return np.array(self._cov, dtype=np.float64).reshape(6, 6)

    @property
    def info(self) -> np.ndarray:
        return np.array(self._info, dtype=np.float64).reshape(6, 6)

    def sigmas(self) -> np.ndarray:
        """square roots of cov's diagonal: metres (3), radians (3)"""
        return np.sqrt(np.diag(self.cov))

    def to_bytes(self) -> bytes:
        return bytes(memoryview(self))


assert C.sizeof(PoseInfo) == POSE_INFO_SIZE


def _pose_info_of(handle, seq):
    rec = PoseInfo()
    rc = load_library().lvt_amd_get_pose_info(handle, int(seq), C.byref(rec))
    if rc < 0:
        raise IndexError(f"lvt_amd_get_pose_info: bad handle or no sequence {seq}")
    return rec


def pose_info_eval(params: LvtParameters, q, p, pts, obs) -> PoseInfo:
    """stage entry: the pose-uncertainty evaluation on caller data (q w x y z unit, either sign; pts n x 3; obs n x 2 float32; n <= 4096)"""
    pod = params.to_pod()
    q = np.ascontiguousarray(q, np.float64).reshape(4); p = np.ascontiguousarray(p, np.float64).reshape(3)
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3); obs = np.ascontiguousarray(obs, np.float32).reshape(-1, 2)
    if len(pts) != len(obs):
        raise ValueError("one observation per point")
    rec = PoseInfo()
    if load_library().lvt_amd_pose_info_eval(C.byref(pod), _p(q), _p(p), _p(pts) if len(pts) else None, _p(obs) if len(pts) else None, len(pts), C.byref(rec)) != 0:
        raise RuntimeError("lvt_amd_pose_info_eval failed")
    return rec


def pose_info_to_ros(cov, R) -> np.ndarray:
    """cov with its rotation part on fixed world axes: M cov M^T, M = blockdiag(I, R) (host code: needs the library, not a GPU)"""
    c = np.ascontiguousarray(cov, np.float64).reshape(36); Rm = np.ascontiguousarray(R, np.float64).reshape(9)
    out = np.zeros(36)
    load_library().lvt_amd_pose_info_to_ros(_p(c), _p(Rm), _p(out))
    return out.reshape(6, 6)


RELOC_CONFIG_SIZE, RELOC_RESULT_SIZE = 32, 192   # LVT_AMD_RELOC_CONFIG_SIZE / _RESULT_SIZE: pinned in the header too


class RelocConfig(C.Structure):
    """lvt_amd_reloc_config (include/lvt_amd_ext.h, RELOCALISATION): n_hypotheses 1 ... 1024, gate_px2 and min_disparity finite and > 0, min_inliers >= 3"""
    _fields_ = [("n_hypotheses", C.c_int), ("gate_px2", C.c_float), ("min_disparity", C.c_float), ("min_inliers", C.c_int), ("seed", C.c_uint64),
                ("dry_run", C.c_int), ("reserved", C.c_int)]

    def __init__(self, n_hypotheses=256, gate_px2=16.0, min_disparity=1.0, min_inliers=30, seed=0, dry_run=0):
        super().__init__(int(n_hypotheses), float(gate_px2), float(min_disparity), int(min_inliers), int(seed), int(dry_run), 0)

    def __repr__(self):
        return (f"RelocConfig(n_hypotheses={self.n_hypotheses}, gate_px2={self.gate_px2}, min_disparity={self.min_disparity}, "
                f"min_inliers={self.min_inliers}, seed={self.seed}, dry_run={self.dry_run})")


class RelocResult(C.Structure):
    """lvt_amd_reloc_result: status 0 = a pose, 1 = fewer than 3 correspondences with a camera-frame point, 2 = the best hypothesis is below the success
    count, 3 = the refined pose is not finite or below the success count; the pose (camera-to-world) is filled for status 0 and 3"""
    _fields_ = [("status", C.c_int), ("n_features", C.c_int), ("n_map", C.c_int), ("n_matched", C.c_int), ("n_corr", C.c_int), ("n_with_point", C.c_int),
                ("best_hypothesis", C.c_int), ("n_hyp_inliers", C.c_int), ("n_refined_inliers", C.c_int), ("reserved", C.c_int),
                ("_q", C.c_double * 4), ("_p", C.c_double * 3), ("_R", C.c_double * 9), ("_t", C.c_double * 3)]

    @property
    def q(self) -> np.ndarray:
        return np.array(self._q, dtype=np.float64)

    @property
    def p(self) -> np.ndarray:
        return np.array(self._p, dtype=np.float64)

    @property
    def R(self) -> np.ndarray:
        return np.array(self._R, dtype=np.float64).reshape(3, 3)

    @property
    def t(self) -> np.ndarray:
        return np.array(self._t, dtype=np.float64)


assert C.sizeof(RelocConfig) == RELOC_CONFIG_SIZE and C.sizeof(RelocResult) == RELOC_RESULT_SIZE


def _reloc_config(cfg, kw) -> RelocConfig:
    if cfg is not None and kw:
        raise TypeError("either a RelocConfig or its fields as keywords, not both")
    if cfg is not None and not isinstance(cfg, RelocConfig):
        raise TypeError("cfg is a RelocConfig")
    return cfg if cfg is not None else RelocConfig(**kw)


def _relocalise(handle, seq, cfg, kw):
    """the RelocResult of lvt_amd_relocalise (seq None) / lvt_amd_batch_relocalise (status 0: relocalised); a refusal raises ValueError with the library's sentence"""
    L = load_library()
    cfg = _reloc_config(cfg, kw)
    res = RelocResult()
    rc = L.lvt_amd_relocalise(handle, C.byref(cfg), C.byref(res)) if seq is None else L.lvt_amd_batch_relocalise(handle, int(seq), C.byref(cfg), C.byref(res))
    if rc < 0:
        raise ValueError((L.lvt_amd_last_error(handle) or b"").decode())
    return res


def reloc_default_config() -> RelocConfig:
    """lvt_amd_reloc_default_config: the library's own defaults (host code: needs the library, not a GPU)"""
    cfg = RelocConfig(0, 0.0, 0.0, 0, 0, 0)
    load_library().lvt_amd_reloc_default_config(C.byref(cfg))
    return cfg


def reloc_slice_length(n_map: int) -> int:
    """points per slice the global matcher cuts a map of n_map points into (host code)"""
    return int(load_library().lvt_amd_reloc_slice_length(int(n_map)))


def reloc_match_device(q_desc, t_desc, out, stream: int = 0) -> float:
    """stage 1 of the relocalisation alone on DEVICE tensors (torch): q_desc (N, 32) u8, t_desc (M, 32) u8, out (N, 4) i32 = (idx1, d1, idx2, d2), -1 / INT_MAX
    where there is none.  Returns the time of the two launches in us."""
    L = load_library()
    us = L.lvt_amd_reloc_match_device(C.c_void_p(q_desc.data_ptr()), int(q_desc.shape[0]), C.c_void_p(t_desc.data_ptr()), int(t_desc.shape[0]),
                                      C.c_void_p(out.data_ptr()), C.c_void_p(stream))
    if us < 0:
        raise RuntimeError("lvt_amd_reloc_match_device failed: " + (L.lvt_amd_last_error(None) or b"").decode())
    return us


def reloc_solve(params: LvtParameters, pts, obs, pc, has_pc, cfg: RelocConfig = None):
    """stages 3 - 5 of the relocalisation alone on caller data: pts n x 3 (world), obs n x 2 float32, pc n x 3 (camera frame), has_pc n bool.  Returns
    (RelocResult, counts (n_hypotheses,), inliers of the best hypothesis, hyp_R (3, 3), hyp_t (3,)); the last two are zero unless status is 0 or 3.
    A refusal raises ValueError with the library's sentence."""
    L = load_library()
    pod = params.to_pod()
    cfg = cfg if cfg is not None else RelocConfig()
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3); obs = np.ascontiguousarray(obs, np.float32).reshape(-1, 2)
    pc = np.ascontiguousarray(pc, np.float64).reshape(-1, 3); has = np.ascontiguousarray(has_pc, np.uint8).reshape(-1)
    n = len(pts)
    if not (len(obs) == len(pc) == len(has) == n):
        raise ValueError("one observation, one camera-frame point and one flag per world point")
    counts = np.zeros(max(int(cfg.n_hypotheses), 1), np.int32); inl = np.zeros(max(n, 1), np.int32); hR = np.zeros(9); ht = np.zeros(3)
    res = RelocResult()
    rc = L.lvt_amd_reloc_solve(C.byref(pod), C.byref(cfg), _p(pts) if n else None, _p(obs) if n else None, _p(pc) if n else None, _p(has) if n else None, n,
                               _p(counts), _p(inl), _p(hR), _p(ht), C.byref(res))
    if rc < 0:
        raise ValueError((L.lvt_amd_last_error(None) or b"").decode())
    return res, counts[:cfg.n_hypotheses].copy(), inl[:max(res.n_hyp_inliers, 0) if res.status in (0, 3) else 0].copy(), hR.reshape(3, 3), ht


RELOC_CAPACITY = 4096                                            # rows of every output array of lvt_amd_reloc_correspond (NF_MAX)
RELOC_SENTINEL_INT, RELOC_SENTINEL_F64, RELOC_SENTINEL_F32, RELOC_SENTINEL_BYTE = -77, -7.7e77, np.float32(-7.7e37), 0xEE


def reloc_correspond(params: LvtParameters, sensor: int, xy_l, desc_l, map_xyz, map_desc, right=None, depth=None, other=None, map_copy: int = 0,
                     lost_frame: int = 0, cfg: RelocConfig = None) -> dict:
    """stage 2 of the relocalisation (behind stage 1) on caller data, through the launches of a handle's call (lvt_amd_reloc_correspond).  xy_l (N, 2) f32,
    desc_l (N, 32) u8; right = (xy_r, desc_r) for stereo; depth (N,) f32 for RGB-D; map_xyz (M, 3) f64, map_desc (M, 32) u8; other = (xyz, desc) of M rows
    for the map copy that is NOT live.  Returns the result record's counts and status, and feat, X, uv, has_pc, pc, with_pc UNTRIMMED (RELOC_CAPACITY rows,
    pre-filled with the RELOC_SENTINEL_* values: what the call does not write keeps them), and claims_left.  A refusal raises ValueError."""
    L = load_library()
    pod = params.to_pod()
    cfg = cfg if cfg is not None else RelocConfig()
    f32 = lambda a, cols: np.ascontiguousarray(a, np.float32).reshape(-1, cols) if a is not None else np.zeros((0, cols), np.float32)
    u8 = lambda a: np.ascontiguousarray(a, np.uint8).reshape(-1, 32) if a is not None else np.zeros((0, 32), np.uint8)
    xy_l, desc_l = f32(xy_l, 2), u8(desc_l)
    xy_r, desc_r = (f32(right[0], 2), u8(right[1])) if right is not None else (f32(None, 2), u8(None))
    xl, yl, xr, yr = (np.ascontiguousarray(a) for a in (xy_l[:, 0], xy_l[:, 1], xy_r[:, 0], xy_r[:, 1]))
    dep = np.ascontiguousarray(depth, np.float32).reshape(-1) if depth is not None else None
    mpos, mdesc = np.ascontiguousarray(map_xyz, np.float64).reshape(-1, 3), u8(map_desc)
    opos, odesc = (np.ascontiguousarray(other[0], np.float64).reshape(-1, 3), u8(other[1])) if other is not None else (None, None)
    n_l, n_r, n_m = len(xy_l), len(xy_r), len(mpos)
    if len(desc_l) != n_l or len(desc_r) != n_r or len(mdesc) != n_m or (dep is not None and len(dep) != n_l) or (opos is not None and not (len(opos) == len(odesc) == n_m)):
        raise ValueError("one descriptor (and one depth) per feature, one descriptor per map point, the other map copy as long as the live one")
    cap = RELOC_CAPACITY
    out = dict(feat=np.full(cap, RELOC_SENTINEL_INT, np.int32), X=np.full((cap, 3), RELOC_SENTINEL_F64), uv=np.full((cap, 2), RELOC_SENTINEL_F32, np.float32),
               has_pc=np.full(cap, RELOC_SENTINEL_BYTE, np.uint8), pc=np.full((cap, 3), RELOC_SENTINEL_F64), with_pc=np.full(cap, RELOC_SENTINEL_INT, np.int32))
    res, left = RelocResult(), C.c_int(-1)
    ptr = lambda a: _p(a) if a is not None and a.size else None
    rc = L.lvt_amd_reloc_correspond(C.byref(pod), C.byref(cfg), int(sensor), ptr(xl), ptr(yl), ptr(desc_l), ptr(dep), n_l, ptr(xr), ptr(yr), ptr(desc_r), n_r,
                                    ptr(mpos), ptr(mdesc), ptr(opos), ptr(odesc), n_m, int(map_copy), int(lost_frame), C.byref(res), _p(out["feat"]), _p(out["X"]),
                                    _p(out["uv"]), _p(out["has_pc"]), _p(out["pc"]), _p(out["with_pc"]), C.byref(left))
    if rc < 0:
        raise ValueError((L.lvt_amd_last_error(None) or b"").decode())
    out.update(status=res.status, n_features=res.n_features, n_map=res.n_map, n_matched=res.n_matched, n_corr=res.n_corr, n_with_point=res.n_with_point,
               claims_left=left.value)
    return out


def _params_of(pod):
    return LvtParameters(**{n: getattr(pod, n) for n, _ in ParamsPOD._fields_ if n in LvtParameters.__dataclass_fields__})


class Snapshot:
    """One sequence's tracker state (control record, map, staged points, motion model), device-resident and owned by the library (lvt_amd_snapshot_*):
    taken from a system or a batch sequence, applied to any number of them, exported to bytes and imported again -- on another device, in another process."""

    def __init__(self, handle):
        self._h = handle

    @property
    def info(self) -> dict:
        """version, sensor_type, state, frame_number, map_n, staged_n, src_map_cur, src_staged_cur, device, bytes (the size of to_bytes())"""
        i = SnapshotInfo()
        if load_library().lvt_amd_snapshot_get_info(self._h, C.byref(i)) != 0:
            raise RuntimeError("lvt_amd_snapshot_get_info failed")
        return i.as_dict()

    @property
    def params(self) -> LvtParameters:
        pod = ParamsPOD()
        if load_library().lvt_amd_snapshot_get_params(self._h, C.byref(pod)) != 0:
            raise RuntimeError("lvt_amd_snapshot_get_params failed")
        return _params_of(pod)

    def to_bytes(self) -> bytes:
        n = self.info["bytes"]
        buf = np.zeros(n, np.uint8)
        if load_library().lvt_amd_snapshot_export(self._h, _p(buf), n) != n:
            raise RuntimeError("lvt_amd_snapshot_export failed")
        return buf.tobytes()

    @classmethod
    def from_bytes(cls, b, device: int = -1) -> "Snapshot":
        """the snapshot these bytes hold, uploaded to `device` (-1: the current one); ValueError with the reason when they are refused"""
        L = load_library()
        a = np.frombuffer(bytes(b), np.uint8)
        h = L.lvt_amd_snapshot_import(_p(a) if a.size else None, a.size, device)
        if not h:
            raise ValueError(L.lvt_amd_last_error(None).decode())
        return cls(h)

    @staticmethod
    def describe(b):
        """(info dict, LvtParameters) of exported bytes -- host code, no GPU needed; ValueError with the reason when they are no snapshot"""
        L = load_library()
        a = np.frombuffer(bytes(b), np.uint8)
        i, pod = SnapshotInfo(), ParamsPOD()
        if L.lvt_amd_snapshot_describe(_p(a) if a.size else None, a.size, C.byref(i), C.byref(pod)) != 0:
            raise ValueError(L.lvt_amd_last_error(None).decode())
        return i.as_dict(), _params_of(pod)

    def close(self):
        if self._h:
            load_library().lvt_amd_snapshot_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class LvtSystem:
    """Mirror of `lvt_system` (reference lvt/src/lvt_system.h:41-109) over the HIP C-ABI."""

    def __init__(self, handle, sensor_type):
        self._h = handle
        self._sensor = sensor_type
        self._bpp = 1   # bytes per pixel of the handle's pixel format (set_pixel_format), or of its sensor format
        self._sfmt = SENSOR_NONE   # the handle's sensor format (set_sensor_format)

    def _img(self, img):
        """a host image as the entry points take it: (H, W) gray, (H, W, bpp) colour, or the sensor's plane (sensor_plane)"""
        return _u8(sensor_plane(img, self._sfmt) if self._sfmt else img, self._bpp)

    # lvt_system::create(const lvt_parameters&, eSensor)  -- lvt_system.cpp:70-127
    @classmethod
    def create(cls, params: LvtParameters, sensor_type: int = eSensor_STEREO, device: int = -1, pooled: bool = False) -> "LvtSystem":
        """device >= 0: the handle owns that HIP device whatever the calling thread's current device is (lvt_amd_create_on_device);
        pooled: a seat of the device's shared lock-step chain (lvt_amd_create_pooled)"""
        L = load_library()
        pod = params.to_pod()
        if pooled:
            h = L.lvt_amd_create_pooled(C.byref(pod), sensor_type, device)
        else:
            h = L.lvt_amd_create_on_device(C.byref(pod), sensor_type, device) if device >= 0 else L.lvt_amd_create(C.byref(pod), sensor_type)
        if not h:
            raise RuntimeError("lvt_amd_create failed (bad parameters, or no usable HIP device -- no CPU fallback)")
        return cls(h, sensor_type)

    # lvt_create(config_file, sensor)  -- lvt_c.cpp:33-48
    @classmethod
    def create_from_file(cls, config_file: str, sensor_type: int = eSensor_STEREO) -> "LvtSystem":
        L = load_library()
        h = L.lvt_create(config_file.encode(), sensor_type)
        if not h:
            raise RuntimeError("lvt_create returned NULL")
        return cls(h, sensor_type)

    @staticmethod
    def destroy(system: "LvtSystem"):
        system.close()

    def close(self):
        if self._h:
            load_library().lvt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        load_library().lvt_amd_reset(self._h)

    def snapshot(self) -> Snapshot:
        """the state after the last frame handed in (drains first); this system goes on tracking.  RuntimeError with the reason when refused"""
        h = load_library().lvt_amd_snapshot_take(self._h, 0)
        if not h:
            raise RuntimeError(self.last_error() or "lvt_amd_snapshot_take failed")
        return Snapshot(h)

    def restore(self, snap: Snapshot) -> int:
        """replace this system's whole state by the snapshot's: the next frame continues the snapshot's trajectory.  0: done; -1: refused (last_error())"""
        return load_library().lvt_amd_snapshot_apply(self._h, 0, snap._h if snap is not None else None)

    def relocalise(self, cfg: RelocConfig = None, **kw) -> RelocResult:
        """lvt_amd_relocalise: search the kept map for the last frame handed in, with no pose prior; status 0 = relocalised (and, unless dry_run, committed:
        the next frame tracks on from the returned pose).  Keywords are RelocConfig fields.  A refusal raises ValueError with the library's sentence."""
        return _relocalise(self._h, None, cfg, kw)

    def get_sensor_type(self):
        return self._sensor

    def device(self) -> int:
        return load_library().lvt_amd_get_device(self._h)

    def get_state(self):
        return load_library().lvt_get_status(self._h)

    def last_error(self) -> str:
        return load_library().lvt_amd_last_error(self._h).decode()

    def host_stats(self) -> dict:
        """host-side counters: frames enqueued / collected, host-buffer planes read in place (page-locked caller buffers) / staged"""
        a = (C.c_longlong * 8)()
        load_library().lvt_amd_get_host_stats(self._h, a)
        return {"enqueued": int(a[0]), "collected": int(a[1]), "planes_in_place": int(a[2]), "planes_staged": int(a[3]),
                "async_host_frames": int(a[4]), "pulls_carried_by_the_previous_frame": int(a[5]), "score_pieces": int(a[6]), "event_ordering": int(a[7])}

    # lvt_system::track(img1, img2)  -- lvt_system.cpp:157-207
    def track(self, img1, img2, depth_scale=None):
        """RGB-D: img2 is the depth image -- floats (metres), or a uint16 array of raw sensor units with depth_scale = metres per unit"""
        R = np.zeros((3, 3)); t = np.zeros(3)
        a = self._img(img1)
        if self._sensor == eSensor_STEREO:
            b = self._img(img2)
            load_library().lvt_track(self._h, _p(a), _p(b), a.shape[0], a.shape[1], _p(R), _p(t))
        elif isinstance(img2, np.ndarray) and img2.dtype == np.uint16:
            if depth_scale is None:
                raise ValueError("a uint16 depth image needs depth_scale (metres per raw unit)")
            d = self._depth(np.ascontiguousarray(img2))
            load_library().lvt_amd_track_rgbd16(self._h, _p(a), _p(d), float(depth_scale), a.shape[0], a.shape[1], _p(R), _p(t))
        else:
            d = self._depth(np.ascontiguousarray(img2, dtype=np.float32))
            load_library().lvt_amd_track_rgbd(self._h, _p(a), _p(d), a.shape[0], a.shape[1], _p(R), _p(t))
        return R, t

    # lvt_system::track_with_external_corners  -- lvt_system.cpp:209-250
    def track_with_external_corners(self, left, right, corners_left, corners_right):
        R = np.zeros((3, 3)); t = np.zeros(3)
        a, b = self._img(left), self._img(right)
        cl = np.ascontiguousarray(corners_left, dtype=np.float64).reshape(-1, 2)
        cr = np.ascontiguousarray(corners_right, dtype=np.float64).reshape(-1, 2)
        load_library().lvt_track_with_external_corners(self._h, _p(a), _p(b), a.shape[0], a.shape[1], _p(cl), len(cl),
                                                       _p(cr), len(cr), _p(R), _p(t))
        return R, t

    # zero-copy: images already resident in HBM (torch uint8 CUDA tensors or raw device pointers)
    def track_device(self, d_left: int, d_right: int, rows: int, cols: int, pitch: int):
        R = np.zeros((3, 3)); t = np.zeros(3)
        load_library().lvt_amd_track_device(self._h, C.c_void_p(d_left), C.c_void_p(d_right), rows, cols, pitch, _p(R), _p(t))
        return R, t

    def track_device_async(self, d_left: int, d_right: int, rows: int, cols: int, pitch: int):
        load_library().lvt_amd_track_device_async(self._h, C.c_void_p(d_left), C.c_void_p(d_right), rows, cols, pitch)

    # RGB-D planes already resident in HBM: gray u8 (16-byte aligned, pitch % 16 == 0) + depth f32 / u16 (pitch in bytes)
    def track_rgbd_device(self, d_gray: int, d_depth: int, rows: int, cols: int, gray_pitch: int, depth_pitch: int, depth_format: int = DEPTH_F32,
                          depth_scale: float = 1.0):
        """(R, t), or None when the frame was refused (last_error() says why; nothing was enqueued)"""
        R = np.zeros((3, 3)); t = np.zeros(3)
        rc = load_library().lvt_amd_track_rgbd_device(self._h, C.c_void_p(d_gray), gray_pitch, C.c_void_p(d_depth), depth_pitch, depth_format,
                                                      float(depth_scale), rows, cols, _p(R), _p(t))
        return (R, t) if rc == 0 else None

    def track_rgbd_device_async(self, d_gray: int, d_depth: int, rows: int, cols: int, gray_pitch: int, depth_pitch: int, depth_format: int = DEPTH_F32,
                                depth_scale: float = 1.0) -> int:
        return load_library().lvt_amd_track_rgbd_device_async(self._h, C.c_void_p(d_gray), gray_pitch, C.c_void_p(d_depth), depth_pitch, depth_format,
                                                              float(depth_scale), rows, cols)

    def track_async(self, img1, img2, depth_scale=None) -> int:
        """lvt_amd_track_async / lvt_amd_track_rgbd_async: HOST images, the call returns once the frame is enqueued (0) or rejected (-1).
        The arrays are used as they are (no copy here): a page-locked one must stay alive and unchanged until the frame is collected."""
        a = self._img(img1)   # (a contiguous uint8 array passes through as it is)
        if self._sensor == eSensor_STEREO:
            b = self._img(img2)
            return load_library().lvt_amd_track_async(self._h, _p(a), _p(b), a.shape[0], a.shape[1])
        if isinstance(img2, np.ndarray) and img2.dtype == np.uint16:
            if depth_scale is None:
                raise ValueError("a uint16 depth image needs depth_scale (metres per raw unit)")
            d = self._depth(img2 if img2.flags.c_contiguous else np.ascontiguousarray(img2))
            return load_library().lvt_amd_track_rgbd16_async(self._h, _p(a), _p(d), float(depth_scale), a.shape[0], a.shape[1])
        d = self._depth(img2 if (isinstance(img2, np.ndarray) and img2.dtype == np.float32 and img2.flags.c_contiguous) else np.ascontiguousarray(img2, dtype=np.float32))
        return load_library().lvt_amd_track_rgbd_async(self._h, _p(a), _p(d), a.shape[0], a.shape[1])

    def track_async_ptr(self, p_left: int, p_right: int, rows: int, cols: int) -> int:
        """the same on raw host addresses (stereo; bench.py: no per-call numpy work inside the timed region)"""
        return load_library().lvt_amd_track_async(self._h, C.c_void_p(p_left), C.c_void_p(p_right), rows, cols)

    def wait(self):
        R = np.zeros((3, 3)); t = np.zeros(3)
        load_library().lvt_amd_wait(self._h, _p(R), _p(t))
        return R, t

    def wait_status(self):
        """(R, t, state after that frame) of the oldest un-collected frame"""
        R = np.zeros((3, 3)); t = np.zeros(3)
        st = load_library().lvt_amd_wait_status(self._h, _p(R), _p(t))
        return R, t, st

    def set_rectifiers(self, left, right) -> int:
        """attach a pair of Rectifier objects (or None, None to detach): every stereo frame handed to this system is then a RAW frame, rectified at the head of
        its feature stage.  The pair's destination (w x h) is this system's image size; its source size (src_w x src_h, the same for both) is the shape every
        frame has from then on -- Rectifier.from_lens makes rectifiers whose source is not the destination's size.  0: done; -1: refused (last_error() says
        why).  The rectifiers are borrowed: keep them alive while they are attached."""
        rc = load_library().lvt_amd_set_rectifiers(self._h, left._h if left is not None else None, right._h if right is not None else None)
        if rc == 0:
            self._rect = (left, right)
        return rc

    def set_pixel_format(self, fmt: int) -> int:
        """PIX_GRAY8 ... PIX_RGBA8: every frame handed to this system from now on is in that format -- host images (H, W, bpp) uint8, device planes with any
        base address and any pitch >= W * bpp; the conversion to gray is the first launch of the frame's feature stage.  0: done; -1: refused (last_error())."""
        rc = load_library().lvt_amd_set_pixel_format(self._h, int(fmt))
        if rc == 0 and not self._sfmt:   # (GRAY8 on a handle with a sensor format is accepted and changes nothing)
            self._bpp = PIX_BPP[int(fmt)]
        return rc

    def pixel_format(self) -> int:
        return load_library().lvt_amd_get_pixel_format(self._h, 0)

    def set_sensor_format(self, cfg=None, **kw) -> int:
        """a SensorFormat (or a SENSOR_* constant, or its arguments: format=, auto_window=, lo=, hi=, lo_permille=, hi_permille=, min_span=): every frame handed
        to this system from now on is the sensor's plane -- a Bayer mosaic (H, W) uint8, YUV 4:2:2 (H, 2 W) uint8, MONO16 (H, W) uint16; device planes at any
        address and any pitch that holds a row -- and is turned into gray by the first launch of the frame's feature stage.  None or SENSOR_NONE: plain
        frames again.  0: done; -1: refused (last_error())."""
        cfg = _sensor_format_arg(cfg, kw)
        rc = load_library().lvt_amd_set_sensor_format(self._h, C.byref(cfg))
        if rc == 0 and (self._sfmt or int(cfg.format)):   # (SENSOR_NONE on a handle without a sensor format is accepted and changes nothing: a colour handle keeps its bpp)
            self._sfmt = int(cfg.format)
            self._bpp = SENSOR_BPP[self._sfmt]
        return rc

    def sensor_format(self):
        """the SensorFormat in force, or None"""
        return _sensor_format_of(self._h, 0)

    def sensor_window(self, eye: int = 0):
        """(lo, hi) the MONO16 image `eye` of the last collected frame was mapped with (a fixed window: the record's), or None"""
        return _sensor_window_of(self._h, 0, eye)

    def set_depth_camera(self, cam) -> int:
        """a DepthCamera: every RGB-D frame handed to this system from now on brings its depth plane as the sensor delivers it -- (cam.height, cam.width),
        float32 or uint16 -- and the feature stage registers it to the gray image; None: registered frames again.  0: done; -1: refused (last_error())."""
        rc = load_library().lvt_amd_set_depth_camera(self._h, C.byref(cam) if cam is not None else None)
        if rc == 0:
            self._depth_shape = (int(cam.height), int(cam.width)) if cam is not None else None
        return rc

    def set_equalisation(self, cfg=None, **kw) -> int:
        """an Equalisation (or its arguments: tiles=, clip_limit=): every frame handed to this system from now on has the gray plane its detector reads
        equalised first, two launches at the head of the feature stage; None: plain frames again.  0: done; -1: refused (last_error())."""
        if cfg is None and kw:
            cfg = Equalisation(**kw)
        return load_library().lvt_amd_set_equalisation(self._h, C.byref(cfg) if cfg is not None else None)

    def equalisation(self):
        """the Equalisation that is set, or None"""
        return _equalisation_of(self._h, 0)

    def set_reduction(self, cfg=None, **kw) -> int:
        """a Reduction (or its arguments: factor=, width=, height=): every frame handed to this system from now on is (height, width) large and is averaged down
        by `factor` by one launch at the head of the feature stage; None or factor 1: frames of the system's own size again.  0: done; -1: refused
        (last_error())."""
        cfg = _reduction_arg(cfg, kw)
        return load_library().lvt_amd_set_reduction(self._h, C.byref(cfg))

    def reduction(self):
        """the Reduction in force, or None"""
        return _reduction_of(self._h, 0)

    def set_mask(self, left=None, right=None) -> int:
        """feature masks, (H, W) uint8 or bool arrays on the pixel grid the detector reads, != 0: key points allowed.  Every frame handed to this system from now
        on loses the key points on masked pixels inside the feature stage (one launch between the gather step and BRIEF).  One eye may be None (no mask for
        it); both None: no masks again.  The arrays are copied before the call returns.  0: done; -1: refused (last_error())."""
        l, r = _mask_of(self._h, 0, left), _mask_of(self._h, 0, right)
        return load_library().lvt_amd_set_mask(self._h, _p(l), _p(r))

    def set_mask_device(self, d_left: int = 0, pitch_left: int = 0, d_right: int = 0, pitch_right: int = 0) -> int:
        """set_mask from planes in HBM (device addresses, any alignment, pitch >= width in bytes; 0: no mask for that eye), copied in the order of the system's
        tracking stream before the call returns"""
        return load_library().lvt_amd_set_mask_device(self._h, C.c_void_p(d_left or None), int(pitch_left), C.c_void_p(d_right or None), int(pitch_right))

    def mask_stats(self):
        """{"kept": (left, right), "dropped": (left, right)} of the last frame's mask launch (an eye without a mask: 0, 0); None without a mask, or when the
        last frame went in before the masks were set"""
        return _mask_stats_of(self._h, 0)

    def set_label_mask(self, cfg=None, **kw) -> int:
        """a LabelMask (or its arguments: label_width=, label_height=, drop=, dilate=): from now on a frame may be handed a label image per eye
        (frame_labels), which the feature stage turns into that frame's mask in one launch; None: no record again.  0: done; -1: refused (last_error())."""
        if cfg is None and kw:
            cfg = LabelMask(**kw)
        return load_library().lvt_amd_set_label_mask(self._h, C.byref(cfg) if cfg is not None else None)

    def label_mask(self):
        """the LabelMask that is set, or None"""
        return _record_of("lvt_amd_get_label_mask", LabelMask, self._h, 0)

    def frame_labels(self, left=None, right=None, pitch_left: int = 0, pitch_right: int = 0) -> int:
        """the label images of the NEXT frame handed to this system, accepted with frames in flight: (label_height, label_width) uint8 arrays, copied before
        the call returns, or device addresses (ints) with their pitches in bytes, read in place until that frame has been collected.  One eye may be None (no
        labels for it); both None clears a pending attachment.  0: done; -1: refused (last_error())."""
        return _frame_labels(self._h, 0, left, right, pitch_left, pitch_right)

    def set_depth_guard(self, cfg=None, **kw) -> int:
        """a DepthGuard (or its arguments: radius=, min_support=, tol_abs=, tol_rel=): every RGB-D frame handed to this system from now on loses the key points
        whose depth sample has too little support around it, one launch directly behind the gather step; None: no guard again.  0: done; -1: refused
        (last_error())."""
        cfg = _depth_guard_arg(cfg, kw)
        return load_library().lvt_amd_set_depth_guard(self._h, C.byref(cfg) if cfg is not None else None)

    def depth_guard(self):
        """the DepthGuard that is set, or None"""
        return _depth_guard_of(self._h, 0)

    def depth_guard_stats(self):
        """{"kept": n, "dropped": n} of the last frame's guard launch; None without a guard, or when the last frame went in before the record was set"""
        return _depth_guard_stats_of(self._h, 0)

    def _depth(self, d):
        """the depth array of a host call: with a depth camera set the library reads cam.height x cam.width elements, and the C-ABI has no size argument for
        them -- an array of any other shape would be read past its end"""
        want = getattr(self, "_depth_shape", None)
        if want is not None and tuple(d.shape) != want:
            raise ValueError(f"a depth image of shape {tuple(d.shape)} on a system whose depth camera delivers {want}")
        return d

    def depth_camera(self):
        """the DepthCamera that is set, or None"""
        return _depth_camera_of(self._h, 0)

    def enable_pose_info(self, on: bool = True) -> int:
        """from the next frame on every tracked frame carries a PoseInfo (one more launch per frame, k_pose_info).  0: done; -1: refused (last_error())"""
        return load_library().lvt_amd_enable_pose_info(self._h, 1 if on else 0)

    def pose_info(self) -> PoseInfo:
        """the record of the frame pose() / counts() answer for; status 0 when there is none (not enabled, first frame, LOST, just reset / restored)"""
        return _pose_info_of(self._h, 0)

    def set_stream(self, hip_stream: int):
        """lvt_amd_set_stream: the tracking chain runs on that HIP stream from the next frame on (torch.cuda.current_stream().cuda_stream; 0: the legacy default
        stream), and work enqueued on it before a frame call completes before the frame's planes are read.  Drains first; a pooled seat ignores the call"""
        load_library().lvt_amd_set_stream(self._h, C.c_void_p(hip_stream))

    # ---- introspection of the last frame (for stage-by-stage parity tests) ----
    def counts(self):
        a = np.zeros(N_COUNTS, dtype=np.int32)
        load_library().lvt_amd_get_counts(self._h, _p(a))
        return {n: int(a[i]) for i, n in enumerate(COUNT_NAMES)}

    def features(self, eye=0, cap=16384):
        xy = np.zeros((cap, 2), np.float32); resp = np.zeros(cap, np.float32); desc = np.zeros((cap, 32), np.uint8)
        n = load_library().lvt_amd_get_features(self._h, eye, _p(xy), _p(resp), _p(desc), cap)
        return xy[:n].copy(), resp[:n].copy(), desc[:n].copy()

    def matches(self, cap=65536):
        fi = np.zeros(cap, np.int32); xyz = np.zeros((cap, 3), np.float64)
        n = load_library().lvt_amd_get_matches(self._h, _p(fi), _p(xyz), cap)
        return fi[:n].copy(), xyz[:n].copy()

    def row_matches(self, cap=16384):
        pr = np.zeros((cap, 2), np.int32)
        n = load_library().lvt_amd_get_row_matches(self._h, _p(pr), cap)
        return pr[:n].copy()

    def map(self, cap=65536):
        xyz = np.zeros((cap, 3)); cnt = np.zeros(cap, np.int32); age = np.zeros(cap, np.int32); desc = np.zeros((cap, 32), np.uint8)
        n = load_library().lvt_amd_get_map(self._h, _p(xyz), _p(cnt), _p(age), _p(desc), cap)
        return xyz[:n].copy(), cnt[:n].copy(), age[:n].copy(), desc[:n].copy()

    def staged(self, cap=65536):
        xyz = np.zeros((cap, 3)); cnt = np.zeros(cap, np.int32); desc = np.zeros((cap, 32), np.uint8)
        n = load_library().lvt_amd_get_staged(self._h, _p(xyz), _p(cnt), _p(desc), cap)
        return xyz[:n].copy(), cnt[:n].copy(), desc[:n].copy()

    def candidate_lists(self, which, cap=None):
        """the last frame's candidate lists as their builders left them (lvt_amd_get_candidate_lists): which = 'map' | 'staged' | 'row'.
        Returns a dict: keys (n x kc uint32, distance << 16 | index), counts (n), proj (n x 2 f32) and vis (n int8) -- the map / staged queries as the
        device used them, empty for 'row' -- and info (the lvt_amd_list_info record as a dict).  Raises ValueError when the library refuses the call."""
        w = LISTS_WHICH[which] if isinstance(which, str) else int(which)
        L = load_library()
        info = np.zeros(8, np.int32)
        if cap is None:   # the size first (a call with no room fills in the record only)
            L.lvt_amd_get_candidate_lists(self._h, w, None, None, None, None, 0, _p(info))
            cap = int(info[6])
        kc = 128
        keys = np.zeros((max(cap, 1), kc), np.uint32); counts = np.zeros(max(cap, 1), np.int32)
        proj = np.zeros((max(cap, 1), 2), np.float32); vis = np.zeros(max(cap, 1), np.int8)
        n = L.lvt_amd_get_candidate_lists(self._h, w, _p(keys), _p(counts), _p(proj), _p(vis), cap, _p(info))
        if n < 0:
            raise ValueError("lvt_amd_get_candidate_lists refused the call (bad handle, a batch, `which` out of range, or cap too small)")
        assert int(info[0]) == kc
        m = 0 if w == LISTS_WHICH["row"] else n
        return {"keys": keys[:n].copy(), "counts": counts[:n].copy(), "proj": proj[:m].copy(), "vis": vis[:m].copy(),
                "info": dict(zip(LIST_INFO_NAMES, (int(v) for v in info[:7])))}

    def pose(self):
        q = np.zeros(4); p = np.zeros(3)
        load_library().lvt_amd_get_pose(self._h, _p(q), _p(p))
        return q, p

    def predicted_pose(self):
        q = np.zeros(4); p = np.zeros(3)
        load_library().lvt_amd_get_predicted_pose(self._h, _p(q), _p(p))
        return q, p

    def profile_enable(self, on: bool = True):
        load_library().lvt_amd_profile_enable(self._h, 1 if on else 0)

    def profile_read(self):
        """[(kernel name, total ms, launches)] accumulated since profile_enable(True)"""
        out = []
        name = C.create_string_buffer(64); ms = C.c_double(0); calls = C.c_long(0)
        for slot in range(64):
            if not load_library().lvt_amd_profile_read(self._h, slot, name, 64, C.byref(ms), C.byref(calls)):
                if slot >= 32:   # (past the last slot; the slots below it may be absent on this handle)
                    break
                continue
            out.append((name.value.decode(), ms.value, calls.value))
        return out

    def ordering(self):
        """'polling' (gates + early stream), 'events' (barriers only) or 'pooled'; see lvt_amd_get_ordering"""
        return ("polling", "events", "pooled")[load_library().lvt_amd_get_ordering(self._h)]

    def timeline(self):
        a = np.zeros(16, dtype=np.int64)
        load_library().lvt_amd_get_timeline(self._h, _p(a))
        return a

    def debug_stamps(self):
        a = np.zeros(32, dtype=np.int64)
        load_library().lvt_amd_get_debug(self._h, _p(a))
        return a

    def plane(self, eye=0, what=0):
        """what=0: corner score map (u8), what=1: 9x9 box sums (u16), what=2: the rectified image of a system with rectifiers (u8; an empty array
        without them), what=3: the converted gray image of a system with a colour pixel format (u8, before rectification; empty on a gray system),
        what=4: the registered depth plane of a system with a depth camera (float32, +inf where nothing landed; empty without one),
        what=5: the equalised image of a system with an equalisation (u8; empty without one), what=6: the tables it was made with (tiles x 256, u8),
        what=7: the eye's feature mask as the system holds it (u8; empty without one);
        returns (rows, pitch) array"""
        cap = 64 << 20
        buf = np.zeros(cap // 8, dtype=np.uint64)
        pitch = C.c_int(0)
        nbytes = load_library().lvt_amd_get_plane(self._h, eye, what, _p(buf), cap, C.byref(pitch))
        if nbytes < 0:
            raise RuntimeError("lvt_amd_get_plane failed")
        raw = buf.view(np.uint8)[:nbytes]
        if nbytes == 0:
            return np.zeros((0, 0), np.uint8)
        a = raw.view(np.float32 if what == 4 else np.uint16 if what == 1 else np.uint8)
        return a.reshape(-1, pitch.value).copy()


class LvtBatch:
    """B independent sequences advanced in lock-step by one launch chain on one GPU (include/lvt_amd_ext.h)."""

    def __init__(self, params, n_sequences: int = None, sensor_type: int = eSensor_STEREO):
        """params: one LvtParameters for all n_sequences sequences -- or a list of them, one per sequence (a MIXED batch: image size, intrinsics,
        detection grid, radii and thresholds per sequence; frames go through track_device_async_mixed)"""
        L = load_library()
        if isinstance(params, (list, tuple)):
            if n_sequences is not None and n_sequences != len(params):
                raise ValueError("n_sequences differs from the number of parameter sets")
            pods = (ParamsPOD * len(params))(*[p.to_pod() for p in params])
            self._h = L.lvt_amd_batch_create_mixed(pods, sensor_type, len(params))
            if not self._h:
                raise RuntimeError("lvt_amd_batch_create_mixed failed (a refused parameter set, or no usable HIP device -- no CPU fallback)")
            self.B, self.mixed = len(params), True
            return
        pod = params.to_pod()
        self._h = L.lvt_amd_batch_create(C.byref(pod), sensor_type, n_sequences)
        if not self._h:
            raise RuntimeError("lvt_amd_batch_create failed (no usable HIP device -- no CPU fallback)")
        self.B, self.mixed = n_sequences, False

    @classmethod
    def create_mixed(cls, params_list, sensor_type: int = eSensor_STEREO) -> "LvtBatch":
        return cls(list(params_list), None, sensor_type)

    def close(self):
        if self._h:
            load_library().lvt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def track_device_async(self, d_left, d_right, rows, cols, pitch):
        a = (C.c_void_p * self.B)(*[int(x) for x in d_left]); b = (C.c_void_p * self.B)(*[int(x) for x in d_right])
        load_library().lvt_amd_batch_track_device_async(self._h, a, b, rows, cols, pitch)

    def track_device_async_mixed(self, d_left, d_right, rows, cols, pitch) -> int:
        """one lock-step step with per-sequence geometry (sequences of length B); d_left[s] None: sequence s has no frame in this step.
        0: enqueued; -1: rejected, nothing enqueued (last_error() says why)"""
        vps = C.c_void_p * self.B
        ints = C.c_int * self.B
        a = vps(*[None if x is None else int(x) for x in d_left])
        b = vps(*[None if x is None else int(x) for x in d_right])
        return load_library().lvt_amd_batch_track_device_async_mixed(self._h, a, b, ints(*[int(x) for x in rows]), ints(*[int(x) for x in cols]),
                                                                    ints(*[int(x) for x in pitch]))

    def track_rgbd_device_async(self, d_gray, d_depth, rows, cols, gray_pitch, depth_pitch, depth_format: int = DEPTH_F32, depth_scale: float = 1.0) -> int:
        """one lock-step step of an RGB-D batch (uniform or mixed): d_gray / d_depth are sequences of length B of device pointers, None for a sequence
        without a frame in this step; rows, cols and the pitches (bytes) are scalars or sequences of length B.  One depth format and scale per call.
        0: enqueued; -1: refused, nothing enqueued (last_error() says why)"""
        vps = C.c_void_p * self.B
        ints = C.c_int * self.B

        def per_seq(v):
            return ints(*([int(v)] * self.B if np.isscalar(v) else [int(x) for x in v]))
        a = vps(*[None if x is None else int(x) for x in d_gray])
        b = vps(*[None if x is None else int(x) for x in d_depth])
        return load_library().lvt_amd_batch_track_rgbd_device_async(self._h, a, b, per_seq(rows), per_seq(cols), per_seq(gray_pitch), per_seq(depth_pitch),
                                                                   int(depth_format), float(depth_scale))

    def set_rectifiers(self, seq: int, left, right) -> int:
        """LvtSystem.set_rectifiers for sequence `seq` of the batch: its frames are raw from then on, the other sequences' are not"""
        rc = load_library().lvt_amd_batch_set_rectifiers(self._h, int(seq), left._h if left is not None else None, right._h if right is not None else None)
        if rc == 0:
            self.__dict__.setdefault("_rect", {})[int(seq)] = (left, right)
        return rc

    def set_pixel_format(self, seq: int, fmt: int) -> int:
        """LvtSystem.set_pixel_format for sequence `seq` of the batch: its planes are colour from then on, the other sequences' are not"""
        return load_library().lvt_amd_batch_set_pixel_format(self._h, int(seq), int(fmt))

    def pixel_format(self, seq: int) -> int:
        return load_library().lvt_amd_get_pixel_format(self._h, int(seq))

    def set_sensor_format(self, seq: int, cfg=None, **kw) -> int:
        """LvtSystem.set_sensor_format for sequence `seq` of the batch: its planes are the sensor's from then on, the other sequences' are not"""
        cfg = _sensor_format_arg(cfg, kw)
        return load_library().lvt_amd_batch_set_sensor_format(self._h, int(seq), C.byref(cfg))

    def sensor_format(self, seq: int):
        return _sensor_format_of(self._h, seq)

    def sensor_window(self, seq: int, eye: int = 0):
        return _sensor_window_of(self._h, seq, eye)

    def set_depth_camera(self, seq: int, cam) -> int:
        """LvtSystem.set_depth_camera for sequence `seq` of the batch: its depth planes are the sensor's from then on, the other sequences' are not"""
        return load_library().lvt_amd_batch_set_depth_camera(self._h, int(seq), C.byref(cam) if cam is not None else None)

    def depth_camera(self, seq: int):
        return _depth_camera_of(self._h, seq)

    def set_equalisation(self, seq: int, cfg=None, **kw) -> int:
        """LvtSystem.set_equalisation for sequence `seq` of the batch: its frames are equalised from then on, the other sequences' are not"""
        if cfg is None and kw:
            cfg = Equalisation(**kw)
        return load_library().lvt_amd_batch_set_equalisation(self._h, int(seq), C.byref(cfg) if cfg is not None else None)

    def equalisation(self, seq: int):
        return _equalisation_of(self._h, seq)

    def set_reduction(self, seq: int, cfg=None, **kw) -> int:
        """LvtSystem.set_reduction for sequence `seq` of the batch: its frames are large from then on, the other sequences' are not"""
        cfg = _reduction_arg(cfg, kw)
        return load_library().lvt_amd_batch_set_reduction(self._h, int(seq), C.byref(cfg))

    def reduction(self, seq: int):
        return _reduction_of(self._h, seq)

    def set_mask(self, seq: int, left=None, right=None) -> int:
        """LvtSystem.set_mask for sequence `seq` of the batch: its key points are filtered from then on, the other sequences' are not"""
        l, r = _mask_of(self._h, seq, left), _mask_of(self._h, seq, right)
        return load_library().lvt_amd_batch_set_mask(self._h, int(seq), _p(l), _p(r))

    def set_mask_device(self, seq: int, d_left: int = 0, pitch_left: int = 0, d_right: int = 0, pitch_right: int = 0) -> int:
        return load_library().lvt_amd_batch_set_mask_device(self._h, int(seq), C.c_void_p(d_left or None), int(pitch_left), C.c_void_p(d_right or None),
                                                            int(pitch_right))

    def mask_stats(self, seq: int):
        return _mask_stats_of(self._h, seq)

    def set_label_mask(self, seq: int, cfg=None, **kw) -> int:
        """LvtSystem.set_label_mask for sequence `seq` of the batch"""
        if cfg is None and kw:
            cfg = LabelMask(**kw)
        return load_library().lvt_amd_batch_set_label_mask(self._h, int(seq), C.byref(cfg) if cfg is not None else None)

    def label_mask(self, seq: int):
        return _record_of("lvt_amd_get_label_mask", LabelMask, self._h, seq)

    def frame_labels(self, seq: int, left=None, right=None, pitch_left: int = 0, pitch_right: int = 0) -> int:
        """LvtSystem.frame_labels for sequence `seq`: the label images of its frame in the NEXT step, whether or not it takes part in it"""
        return _frame_labels(self._h, seq, left, right, pitch_left, pitch_right)

    def set_depth_guard(self, seq: int, cfg=None, **kw) -> int:
        """LvtSystem.set_depth_guard for sequence `seq` of an RGB-D batch: its key points are guarded from then on, the other sequences' are not"""
        cfg = _depth_guard_arg(cfg, kw)
        return load_library().lvt_amd_batch_set_depth_guard(self._h, int(seq), C.byref(cfg) if cfg is not None else None)

    def depth_guard(self, seq: int):
        return _depth_guard_of(self._h, seq)

    def depth_guard_stats(self, seq: int):
        return _depth_guard_stats_of(self._h, seq)

    def enable_pose_info(self, on: bool = True) -> int:
        """LvtSystem.enable_pose_info for all sequences of the batch together"""
        return load_library().lvt_amd_enable_pose_info(self._h, 1 if on else 0)

    def pose_info(self, seq: int) -> PoseInfo:
        """sequence `seq`'s record of the last collected step (IndexError: no such sequence)"""
        return _pose_info_of(self._h, seq)

    def params(self, seq: int) -> LvtParameters:
        pod = ParamsPOD()
        if not load_library().lvt_amd_batch_get_params(self._h, seq, C.byref(pod)):
            raise IndexError(f"no sequence {seq} in this batch")
        return _params_of(pod)

    def snapshot(self, seq: int = None):
        """the state of sequence `seq` -- or, None, of every sequence through one drain and one launch: a list.  RuntimeError with the reason when refused"""
        L = load_library()
        if seq is not None:
            h = L.lvt_amd_snapshot_take(self._h, int(seq))
            if not h:
                raise RuntimeError(self.last_error() or "lvt_amd_snapshot_take failed")
            return Snapshot(h)
        out = (C.c_void_p * self.B)()
        if L.lvt_amd_batch_snapshot_take(self._h, out) != 0:
            raise RuntimeError(self.last_error() or "lvt_amd_batch_snapshot_take failed")
        return [Snapshot(out[s]) for s in range(self.B)]

    def restore(self, seq: int, snap: Snapshot) -> int:
        """LvtSystem.restore for sequence `seq`; the other sequences are untouched.  0: done; -1: refused (last_error())"""
        return load_library().lvt_amd_snapshot_apply(self._h, int(seq), snap._h if snap is not None else None)

    def restore_all(self, snaps) -> int:
        """one snapshot per sequence (None: leave that sequence alone) through one launch.  0: done; -1: refused, nothing changed (last_error())"""
        if len(snaps) != self.B:
            raise ValueError("one entry per sequence")
        arr = (C.c_void_p * self.B)(*[None if x is None else x._h for x in snaps])
        return load_library().lvt_amd_batch_snapshot_apply(self._h, arr)

    def relocalise(self, seq: int, cfg: RelocConfig = None, **kw) -> RelocResult:
        """lvt_amd_batch_relocalise: LvtSystem.relocalise for sequence seq alone; its neighbours are untouched"""
        return _relocalise(self._h, seq, cfg, kw)

    def reset(self, seq: int) -> int:
        """lvt_system::reset for sequence `seq` alone (drains first).  0: done; -1: refused (last_error())"""
        return load_library().lvt_amd_batch_reset(self._h, int(seq))

    set_stream = LvtSystem.set_stream   # (one stream for the whole batch)

    def wait(self):
        R = np.zeros((self.B, 3, 3)); t = np.zeros((self.B, 3)); st = np.zeros(self.B, np.int32)
        load_library().lvt_amd_batch_wait(self._h, _p(R), _p(t), _p(st))
        return R, t, st

    def counts(self, seq):
        a = np.zeros(N_COUNTS, dtype=np.int32)
        load_library().lvt_amd_batch_get_counts(self._h, seq, _p(a))
        return {n: int(a[i]) for i, n in enumerate(COUNT_NAMES)}

    def last_error(self) -> str:
        return load_library().lvt_amd_last_error(self._h).decode()

    def profile_enable(self, on: bool = True):
        load_library().lvt_amd_profile_enable(self._h, 1 if on else 0)

    profile_read = LvtSystem.profile_read
    timeline = LvtSystem.timeline   # (sequence 0's stamps)
    host_stats = LvtSystem.host_stats
    debug_stamps = LvtSystem.debug_stamps


def mixed_tables(params_list, sensor_type: int = eSensor_STEREO):
    """(cells, score): the work tables a mixed batch of these parameters launches k_cells_mixed / k_score_mixed from (uint32 arrays, one entry per
    workgroup; include/lvt_amd_ext.h, lvt_amd_batch_mixed_tables).  Host code: needs the library, not a GPU.  None: refused parameters."""
    L = load_library()
    pods = (ParamsPOD * len(params_list))(*[p.to_pod() for p in params_list])
    n = np.zeros(2, np.int32)
    if not L.lvt_amd_batch_mixed_tables(pods, sensor_type, len(params_list), None, 0, None, 0, _p(n)):
        return None
    cells, score = np.zeros(int(n[0]), np.uint32), np.zeros(int(n[1]), np.uint32)
    L.lvt_amd_batch_mixed_tables(pods, sensor_type, len(params_list), _p(cells), len(cells), _p(score), len(score), _p(n))
    return cells, score


def _pnp_inputs(params, q_in, p_in, pts, obs):
    """what lvt_amd_pnp, _pnp_detail and _pnp_trace are called with: the library, the parameter record and the four arrays as the C ABI reads them"""
    return (load_library(), params.to_pod(), np.ascontiguousarray(q_in, np.float64), np.ascontiguousarray(p_in, np.float64),
            np.ascontiguousarray(pts, np.float64), np.ascontiguousarray(obs, np.float32))


def pnp(params: LvtParameters, q_in, p_in, pts, obs):
    """stage entry: motion-only BA on caller data (reference lvt_pnp_solver.cpp:60-128)"""
    L, pod, q_in, p_in, pts, obs = _pnp_inputs(params, q_in, p_in, pts, obs)
    q = np.zeros(4); p = np.zeros(3); calls = C.c_int(0)
    inl = L.lvt_amd_pnp(C.byref(pod), _p(q_in), _p(p_in), _p(pts), _p(obs), len(pts), _p(q), _p(p), C.byref(calls))
    if inl < 0:
        raise RuntimeError("lvt_amd_pnp failed")
    return q, p, inl, calls.value


def pnp_detail(params: LvtParameters, q_in, p_in, pts, obs):
    """lvt_amd_pnp with the chi2 gates laid open: (q, p, inliers, solve calls, err (n x 2: what the second gate saw), level (n: 1 = demoted),
    borderline = gate decisions taken within 1e-8 of the threshold)"""
    L, pod, q_in, p_in, pts, obs = _pnp_inputs(params, q_in, p_in, pts, obs)
    n = len(pts)
    q = np.zeros(4); p = np.zeros(3); calls = C.c_int(0); border = C.c_int(0)
    err = np.zeros((n, 2)); level = np.zeros(n, np.int32)
    inl = L.lvt_amd_pnp_detail(C.byref(pod), _p(q_in), _p(p_in), _p(pts), _p(obs), n, _p(q), _p(p), C.byref(calls), _p(err), _p(level), C.byref(border))
    if inl < 0:
        raise RuntimeError("lvt_amd_pnp_detail failed")
    return q, p, inl, calls.value, err, level, border.value


def pnp_trace(params: LvtParameters, q_in, p_in, pts, obs, trace_cap=256):
    """lvt_amd_pnp_trace: (q, p, inliers, solve calls, trace rows (trials x 4: lambda, chi2 at the estimate, chi2 of the trial, rho),
    (trials, rejections, terminates))"""
    L, pod, q_in, p_in, pts, obs = _pnp_inputs(params, q_in, p_in, pts, obs)
    q = np.zeros(4); p = np.zeros(3); calls = C.c_int(0)
    tr = np.zeros((trace_cap, 4)); st = np.zeros(3, np.int32)
    inl = L.lvt_amd_pnp_trace(C.byref(pod), _p(q_in), _p(p_in), _p(pts), _p(obs), len(pts), _p(q), _p(p), C.byref(calls), None, None, None,
                              _p(tr), trace_cap, _p(st))
    if inl < 0:
        raise RuntimeError("lvt_amd_pnp_trace failed")
    return q, p, inl, calls.value, tr[:min(int(st[0]), trace_cap)].copy(), tuple(int(x) for x in st)


def motion_predict(state, q, p):
    """stage entry: the constant-velocity motion model on caller data (reference lvt_motion_model.cpp:42-65), one device thread through the frame path's own
    motion_predict.  state = last_q[4] (w x y z), ang_vel[4], last_p[3], lin_vel[3]; returns (next state[14], predicted q, predicted p)"""
    st = np.ascontiguousarray(state, np.float64).reshape(14).copy()
    q = np.ascontiguousarray(q, np.float64).reshape(4); p = np.ascontiguousarray(p, np.float64).reshape(3)
    qo = np.zeros(4); po = np.zeros(3)
    if load_library().lvt_amd_motion_predict(_p(st), _p(q), _p(p), _p(qo), _p(po)) != 0:
        raise RuntimeError("lvt_amd_motion_predict failed")
    return st, qo, po


def hamming_match_batched(q_desc, q_xy, t_desc, t_xy, t_flag, r2: float, mode: int, img_rows: int, img_cols: int, out, stream: int = 0,
                          launches: int = 1):
    """Batched masked 2-NN Hamming matcher on DEVICE tensors (torch): q_desc (B,M,32) u8, q_xy (B,M,2) f32,
    t_desc (B,N,32) u8, t_xy (B,N,2) f32, t_flag (B,N) u8, out (B,M,4) i32.  Returns kernel time in us."""
    L = load_library()
    B, M = q_desc.shape[0], q_desc.shape[1]
    N = t_desc.shape[1]
    us = L.lvt_amd_hamming_match_batched_n(C.c_void_p(q_desc.data_ptr()), C.c_void_p(q_xy.data_ptr()), C.c_void_p(t_desc.data_ptr()),
                                           C.c_void_p(t_xy.data_ptr()), C.c_void_p(t_flag.data_ptr()), B, M, N, float(r2), int(mode),
                                           int(img_rows), int(img_cols), C.c_void_p(out.data_ptr()), C.c_void_p(stream), int(launches))
    if us < 0:
        raise RuntimeError("lvt_amd_hamming_match_batched failed")
    return us  # (0.0 for an empty train set: nothing was timed)


def remap_device(d_src: int, sw: int, sh: int, src_pitch: int, map1, map2, d_dst: int, dst_pitch: int, route: int = 0):
    """stage entry: the rectifier's remap alone ("RECTIFICATION", include/lvt_amd_ext.h).  d_src / d_dst are device addresses (u8 planes of sh x src_pitch and
    dh x dst_pitch bytes), map1 / map2 host float32 arrays of one shape (dh, dw), which need not be the source's; route 0 = k_rectify, route 1 = k_rectify_fix +
    k_rectify_frames.  Returns (rc, kernels launched): (0, 1 or 2), or (-1, 0) on a refusal, whose sentence is last_call_error()."""
    m1 = np.ascontiguousarray(map1, np.float32); m2 = np.ascontiguousarray(map2, np.float32)
    if m1.ndim != 2 or m1.shape != m2.shape:
        raise ValueError("map1 and map2 must be two-dimensional and of one shape")
    n = C.c_int(-1)
    rc = load_library().lvt_amd_remap_device(C.c_void_p(d_src), int(sw), int(sh), int(src_pitch), _p(m1), _p(m2), m1.shape[1], m1.shape[0], C.c_void_p(d_dst),
                                             int(dst_pitch), int(route), C.byref(n))
    return rc, n.value


def last_call_error() -> str:
    """the sentence of the calling thread's last refused handle-less call (lvt_amd_last_error(NULL))"""
    return (load_library().lvt_amd_last_error(None) or b"").decode()


LENS_RADTAN, LENS_FISHEYE = 0, 1   # LVT_AMD_LENS_*


class _LensRecord(C.Structure):   # lvt_amd_lens
    _fields_ = [("model", C.c_int), ("width", C.c_int), ("height", C.c_int), ("K", C.c_double * 9), ("D", C.c_double * 12)]


class Lens:
    """lvt_amd_lens ("LENS MODELS", include/lvt_amd_ext.h): the model (LENS_RADTAN / LENS_FISHEYE), the RAW image's size, K (3 x 3) and the distortion
    coefficients -- RADTAN: up to 12 in OpenCV's order k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4, FISHEYE: k1 k2 k3 k4; a shorter D is padded with zeros."""

    def __init__(self, model: int, width: int, height: int, K, D):
        D = np.asarray(D, np.float64).reshape(-1)
        if D.size > 12:
            raise ValueError(f"a lens has at most 12 distortion coefficients, not {D.size}")
        self.model, self.width, self.height = int(model), int(width), int(height)
        self.K = np.array(K, np.float64).reshape(3, 3)
        self.D = np.concatenate([D, np.zeros(12 - D.size)])

    def _record(self) -> _LensRecord:
        return _LensRecord(self.model, self.width, self.height, (C.c_double * 9)(*self.K.reshape(-1)), (C.c_double * 12)(*self.D))

    def reduced(self, f: int) -> "Lens":
        """lvt_amd_lens_reduced: the lens of this image reduced by f (a Reduction's geometry); host code, needs the library and no GPU"""
        rec, out = self._record(), _LensRecord()
        if load_library().lvt_amd_lens_reduced(C.byref(rec), int(f), C.byref(out)) != 0:
            raise ValueError(f"lvt_amd_lens_reduced refused factor {f} on a lens of {self.width} x {self.height}")
        return Lens(out.model, out.width, out.height, list(out.K), list(out.D))

    def __repr__(self):
        return f"Lens(model={self.model}, width={self.width}, height={self.height}, K={self.K.tolist()}, D={self.D.tolist()})"


class Rectifier:
    """cv::initUndistortRectifyMap + cv::remap(INTER_LINEAR) on the GPU (the EuRoC example's pre-step).  w x h is the DESTINATION (the
    rectified image, the maps), src_w x src_h the SOURCE (the raw image): equal for Rectifier(...), the lens's own size for Rectifier.from_lens(...)."""

    def __init__(self, K, D, R, P, width: int, height: int):
        L = load_library()
        a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (K, D, R, P)]
        self._keep = a
        self.w, self.h = width, height
        self.src_w, self.src_h = width, height
        self._h = L.lvt_amd_rectifier_create(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), width, height)
        if not self._h:
            raise RuntimeError("lvt_amd_rectifier_create returned NULL")

    @classmethod
    def from_lens(cls, lens: "Lens", R, P, dst_width: int, dst_height: int) -> "Rectifier":
        """lvt_amd_rectifier_create_lens: a RADTAN (up to twelve coefficients) or FISHEYE lens, a raw image of lens.width x lens.height rectified to
        dst_width x dst_height.  ValueError with the library's sentence when the record is refused."""
        L = load_library()
        self = cls.__new__(cls)
        self._h = None
        rec = lens._record()
        a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (R, P)]
        if a[0].size != 9 or a[1].size != 9:
            raise ValueError("R and P are 3 x 3")
        self._keep = a
        self.w, self.h = int(dst_width), int(dst_height)
        self.src_w, self.src_h = lens.width, lens.height
        self._h = L.lvt_amd_rectifier_create_lens(C.byref(rec), _p(a[0]), _p(a[1]), self.w, self.h)
        if not self._h:
            raise ValueError(last_call_error() or "lvt_amd_rectifier_create_lens returned NULL")
        return self

    def info(self):
        """(Lens, (dst_width, dst_height)): the record this rectifier was made from (lvt_amd_rectifier_get_info)"""
        rec, size = _LensRecord(), (C.c_int * 2)()
        if load_library().lvt_amd_rectifier_get_info(self._h, C.byref(rec), size) != 0:
            raise RuntimeError("lvt_amd_rectifier_get_info failed")
        return Lens(rec.model, rec.width, rec.height, list(rec.K), list(rec.D)), (int(size[0]), int(size[1]))

    def maps(self):
        m1 = np.zeros((self.h, self.w), np.float32); m2 = np.zeros((self.h, self.w), np.float32)
        if load_library().lvt_amd_rectifier_get_maps(self._h, _p(m1), _p(m2)) != 0:
            raise RuntimeError("lvt_amd_rectifier_get_maps failed")
        return m1, m2

    def rectify(self, img):
        """a raw (src_h, src_w) image -> the rectified (h, w) one"""
        a = _u8(img)
        if a.shape != (self.src_h, self.src_w):
            raise ValueError(f"a raw image of {a.shape[1]} x {a.shape[0]} for a rectifier whose source is {self.src_w} x {self.src_h}")
        out = np.zeros((self.h, self.w), np.uint8)
        if load_library().lvt_amd_rectify(self._h, _p(a), _p(out)) != 0:
            raise RuntimeError("lvt_amd_rectify failed")
        return out

    def rectify_device(self, d_src: int, src_pitch: int, d_dst: int, dst_pitch: int, stream: int = 0) -> int:
        """stage entry: the remap alone on device planes, enqueued on `stream` (u8; src_pitch >= the source's width; dst_pitch % 4 == 0 and >= width: every byte of
        height x dst_pitch is written, the columns from width on as zero); 0 / -1 (refused, nothing enqueued)"""
        return load_library().lvt_amd_rectify_device(self._h, C.c_void_p(d_src), int(src_pitch), C.c_void_p(d_dst), int(dst_pitch), C.c_void_p(stream))

    def close(self):
        if self._h:
            load_library().lvt_amd_rectifier_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class Odometry:
    """What the reference's ROS node does with every pose (lvt_ros.cpp:215-311), without ROS: x-forward / z-up re-expression,
    base-frame deltas accumulated into base_to_odom, stale frames ignored, tracker (+ optionally pose) reset on LOST."""

    def __init__(self, system=None, base_to_sensor=None, reset_pose_on_lost=True):
        L = load_library()
        self._sys = system
        b = None if base_to_sensor is None else np.ascontiguousarray(base_to_sensor, dtype=np.float64).reshape(12)
        self._h = L.lvt_amd_odometry_create(system._h if system is not None else None, None if b is None else _p(b), 1 if reset_pose_on_lost else 0)
        if not self._h:
            raise RuntimeError("lvt_amd_odometry_create returned NULL")

    def _call(self, fn, *args):
        pose = np.zeros(7); twist = np.zeros(6)
        rc = fn(self._h, *args, _p(pose), _p(twist))
        if rc < 0:
            raise ValueError("bad arguments")
        return (pose, twist) if rc == 1 else None

    def set_relocalisation(self, cfg: RelocConfig = None, max_lost_frames: int = 10, **kw) -> int:
        """lvt_amd_odometry_set_relocalisation: on a LOST frame relocalise the tracker instead of resetting it; after max_lost_frames failures in a row the
        reference's reset.  max_lost_frames <= 0 turns the policy off.  A bad config field raises ValueError with the library's sentence."""
        L = load_library()
        if L.lvt_amd_odometry_set_relocalisation(self._h, C.byref(_reloc_config(cfg, kw)), int(max_lost_frames)) != 0:
            raise ValueError((L.lvt_amd_last_error(None) or b"").decode())
        return 0

    def push_pose(self, R, t, status, stamp):
        """returns (pose[x y z qx qy qz qw], twist[6]) or None (LOST -> reset, or a stale time stamp)"""
        Rm = np.ascontiguousarray(R, dtype=np.float64).reshape(3, 3); tv = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        return self._call(load_library().lvt_amd_odometry_push_pose, _p(Rm), _p(tv), int(status), float(stamp))

    def update(self, left, right, stamp):
        a, b = _u8(left), _u8(right)
        return self._call(load_library().lvt_amd_odometry_update, _p(a), _p(b), a.shape[0], a.shape[1], float(stamp))

    def _call_cov(self, fn, *args):
        pose = np.zeros(7); twist = np.zeros(6); cov = np.zeros(36)
        rc = fn(self._h, *args, _p(pose), _p(twist), _p(cov))
        if rc < 0:
            raise ValueError("bad arguments")
        return (pose, twist, cov.reshape(6, 6)) if rc == 1 else None

    def push_pose_cov(self, R, t, status, stamp, cov=None):
        """push_pose with the 6 x 6 covariance of the published pose (ROS order, rotation about odom's fixed axes): (pose, twist, cov_out) or None.
        cov: the frame's PoseInfo.cov (hand in None unless its status is 1); None gives zeros"""
        Rm = np.ascontiguousarray(R, dtype=np.float64).reshape(3, 3); tv = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        c = None if cov is None else np.ascontiguousarray(cov, dtype=np.float64).reshape(36)
        pose = np.zeros(7); twist = np.zeros(6); out = np.zeros(36)
        rc = load_library().lvt_amd_odometry_push_pose_cov(self._h, _p(Rm), _p(tv), int(status), float(stamp), _p(c), _p(pose), _p(twist), _p(out))
        if rc < 0:
            raise ValueError("bad arguments")
        return (pose, twist, out.reshape(6, 6)) if rc == 1 else None

    def update_cov(self, left, right, stamp):
        """update with the covariance of the published pose (zeros unless the system has pose info enabled and the frame's record is valid)"""
        a, b = _u8(left), _u8(right)
        return self._call_cov(load_library().lvt_amd_odometry_update_cov, _p(a), _p(b), a.shape[0], a.shape[1], float(stamp))

    def reset(self):
        load_library().lvt_amd_odometry_reset(self._h)

    def close(self):
        if self._h:
            load_library().lvt_amd_odometry_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
