"""CPU tier: lvt_amd_snapshot_describe is host code -- it needs the library, not a device -- and refuses bytes that are no snapshot, with a reason.
(What it accepts is checked on the GPU tier, where snapshots exist: tests/test_gpu_snapshots.py.)"""
import ctypes

import numpy as np
import pytest

SNAP_MAGIC = b"LVT_SNP1"   # the first eight bytes of an exported snapshot (lvt_amd/csrc/k_state.hip)


def _describe_rc(L, raw):
    a = np.frombuffer(raw, np.uint8)
    info = (ctypes.c_byte * 64)()
    return L.lvt_amd_snapshot_describe(a.ctypes.data_as(ctypes.c_void_p) if a.size else None, a.size, info, None)


@pytest.mark.parametrize("n", [0, 16, 4096])
def test_describe_refuses_bytes_that_are_no_snapshot(hip_lib, n):
    raw = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    L = hip_lib.load_library()
    assert _describe_rc(L, raw) == -1
    why = L.lvt_amd_last_error(None).decode()
    assert why.startswith("lvt_amd_snapshot_describe: ") and len(why) > 30, why
    with pytest.raises(ValueError) as e:
        hip_lib.Snapshot.describe(raw)
    assert str(e.value) == why


def test_each_header_check_names_its_reason(hip_lib):
    L = hip_lib.load_library()
    rng = np.random.default_rng(7)
    short = SNAP_MAGIC + bytes(8)
    assert _describe_rc(L, short) == -1 and "too short" in L.lvt_amd_last_error(None).decode()
    no_magic = rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()
    assert no_magic[:8] != SNAP_MAGIC
    assert _describe_rc(L, no_magic) == -1 and "magic" in L.lvt_amd_last_error(None).decode()
    other_version = SNAP_MAGIC + (99).to_bytes(4, "little") + bytes(4084)
    assert _describe_rc(L, other_version) == -1 and "version 99" in L.lvt_amd_last_error(None).decode()
    other_build = SNAP_MAGIC + (1).to_bytes(4, "little") + bytes(4084)      # version 1 with a header size of 0
    assert _describe_rc(L, other_build) == -1 and "another build" in L.lvt_amd_last_error(None).decode()


def test_import_refuses_them_before_it_touches_a_device(hip_lib):
    for raw in (b"", bytes(16), SNAP_MAGIC + bytes(4088)):
        with pytest.raises(ValueError) as e:
            hip_lib.Snapshot.from_bytes(raw)
        assert str(e.value).startswith("lvt_amd_snapshot_import: ")


def test_the_abi_list_names_the_snapshot_calls(hip_lib):
    want = {"lvt_amd_snapshot_take", "lvt_amd_snapshot_apply", "lvt_amd_batch_snapshot_take", "lvt_amd_batch_snapshot_apply", "lvt_amd_snapshot_get_info",
            "lvt_amd_snapshot_get_params", "lvt_amd_snapshot_export", "lvt_amd_snapshot_import", "lvt_amd_snapshot_describe", "lvt_amd_snapshot_destroy",
            "lvt_amd_batch_reset"}
    assert want <= set(hip_lib.ABI_SYMBOLS)
    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    assert all(hasattr(lib, s) for s in want)
    assert ctypes.sizeof(hip_lib.SnapshotInfo) == 48
