"""-m gpu: the stage entries through the C ABI itself (ctypes on lvt_amd.load_library()), on the paths the Python wrappers never take: optional outputs left
NULL, a NULL config, n = 0 with NULL data pointers, and the refusals with their sentences.  An optional output must change nothing else: a call without it
is compared bit for bit with the call that asks for everything.  The n = 0 answers are the ones include/lvt_amd_ext.h writes down."""
import ctypes as C

import numpy as np
import pytest

import lvt_amd
import reloc_cases as RC
from case_tables import pnp_edge_case
from lvt_amd import RelocConfig, RelocResult, _p
from test_gpu_relocalisation import problem

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
NO_HANDLE = b"no handle (creation failed: bad parameters, or no HIP device -- there is no CPU fallback)"


@pytest.fixture(scope="module")
def L(hip_lib):
    return hip_lib.load_library()


def _last(L):
    return (L.lvt_amd_last_error(None) or b"").decode()


# ---- lvt_amd_pnp_trace -----------------------------------------------------------------------------------------------------------------------------------
TRACE_CAP = 64


def _pnp_trace(L, prm, X, uv, q0, p0, err=False, level=False, rest=False):
    """one call; the optional outputs that are not asked for are NULL (rest: borderline, trace and stats)"""
    n = len(X)
    pod = prm.to_pod()
    X = np.ascontiguousarray(X, np.float64); uv = np.ascontiguousarray(uv, np.float32)
    q = np.full(4, -7.0); p = np.full(3, -7.0); calls = C.c_int(-7); border = C.c_int(-7)
    e = np.full((n, 2), -7.0); lv = np.full(n, -7, np.int32); tr = np.full((TRACE_CAP, 4), -7.0); st = np.full(3, -7, np.int32)
    rc = L.lvt_amd_pnp_trace(C.byref(pod), _p(q0), _p(p0), _p(X), _p(uv), n, _p(q), _p(p), C.byref(calls), _p(e) if err else None, _p(lv) if level else None,
                             C.byref(border) if rest else None, _p(tr) if rest else None, TRACE_CAP if rest else 0, _p(st) if rest else None)
    return dict(rc=rc, q=q, p=p, calls=calls.value, err=e, level=lv, border=border.value, trace=tr, stats=st)


@pytest.fixture(scope="module")
def pnp_full(L):
    prm, X, uv, q0, p0 = pnp_edge_case("kitti", 16)
    full = _pnp_trace(L, prm, X, uv, q0, p0, err=True, level=True, rest=True)
    assert full["rc"] > 0 and full["calls"] > 0 and 0 < full["stats"][0] <= TRACE_CAP
    assert (full["err"] != -7.0).all() and set(full["level"]) <= {0, 1} and (full["trace"][:full["stats"][0]] != -7.0).all()
    return (prm, X, uv, q0, p0), full


@pytest.mark.parametrize("asked", ["nothing", "err", "level"])
def test_pnp_trace_optional_outputs_change_nothing_else(L, pnp_full, asked):
    """every optional output NULL and trace_cap = 0 / err_out alone / level_out alone against the call with all of them, 16 points: q, p, the return value
    and n_solve_calls bit for bit, and the one output that was asked for equal to the full call's"""
    case, full = pnp_full
    got = _pnp_trace(L, *case, err=asked == "err", level=asked == "level")
    assert got["rc"] == full["rc"] and got["calls"] == full["calls"]
    assert got["q"].tobytes() == full["q"].tobytes() and got["p"].tobytes() == full["p"].tobytes()
    assert got["err"].tobytes() == (full["err"] if asked == "err" else np.full((16, 2), -7.0)).tobytes()
    assert np.array_equal(got["level"], full["level"] if asked == "level" else np.full(16, -7, np.int32))
    assert got["border"] == -7 and (got["trace"] == -7.0).all() and (got["stats"] == -7).all()


# ---- lvt_amd_reloc_solve ---------------------------------------------------------------------------------------------------------------------------------
def _solve(L, prm, X, uv, pc, has, cfg, outputs=True, n=None):
    n = len(X) if n is None else n
    pod = prm.to_pod()
    X = np.ascontiguousarray(X, np.float64); uv = np.ascontiguousarray(uv, np.float32); pc = np.ascontiguousarray(pc, np.float64)
    has = np.ascontiguousarray(has, np.uint8)
    counts = np.full(1024, -7, np.int32); inl = np.full(max(n, 1), -7, np.int32); hR = np.full(9, -7.0); ht = np.full(3, -7.0)
    res = RelocResult()
    C.memset(C.byref(res), 0xEE, C.sizeof(res))
    data = [_p(a) if len(a) else None for a in (X, uv, pc, has)]
    rc = L.lvt_amd_reloc_solve(C.byref(pod), C.byref(cfg) if cfg is not None else None, *data, n, *([_p(counts), _p(inl), _p(hR), _p(ht)] if outputs else [None] * 4),
                               C.byref(res))
    return rc, bytes(res), res, counts, inl, hR, ht


def test_reloc_solve_without_optional_outputs_and_without_a_config(L):
    """counts_out, inliers_out, hyp_R and hyp_t NULL, and cfg NULL, against the full call with the default config spelled out, 64 correspondences of which
    a fifth are gross outliers: the result record byte for byte, and the return value"""
    prm, X, uv, pc, has, _ = problem(5, 64, outliers=0.2)
    rc, rec, res, counts, inl, hR, ht = _solve(L, prm, X, uv, pc, has, RelocConfig())
    assert rc == 0 and res.status == 0 and res.n_corr == 64 and res.n_hyp_inliers >= 30           # the case runs all of stages 3 - 5
    assert (counts[:256] >= 0).all() and (counts[256:] == -7).all() and (inl[:res.n_hyp_inliers] >= 0).all() and (hR != -7.0).all() and (ht != -7.0).all()
    for cfg, outputs in ((RelocConfig(), False), (None, True), (None, False)):
        rc2, rec2 = _solve(L, prm, X, uv, pc, has, cfg, outputs)[:2]
        assert rc2 == rc and rec2 == rec, (cfg, outputs)


# ---- lvt_amd_reloc_correspond ----------------------------------------------------------------------------------------------------------------------------
def _correspond(L, case, other, claims, prm=None):
    """the stereo case through the entry; other: None (NULL pointers) or (pos, desc); claims: whether claims_left is asked for"""
    pod = (prm or case["prm"]).to_pod()
    cfg = RelocConfig(min_disparity=case["min_disparity"])
    (xy_l, desc_l), (xy_r, desc_r) = (case["xy_l"], case["desc_l"]), case["right"]
    xl, yl, xr, yr = (np.ascontiguousarray(a) for a in (xy_l[:, 0], xy_l[:, 1], xy_r[:, 0], xy_r[:, 1]))
    cap = lvt_amd.RELOC_CAPACITY
    out = [np.full(cap, -77, np.int32), np.full((cap, 3), -7.7e77), np.full((cap, 2), -7.7e37, np.float32), np.full(cap, 0xEE, np.uint8), np.full((cap, 3), -7.7e77),
           np.full(cap, -77, np.int32)]                                                            # corr_feat, X, uv, has_pc, Pc, with_pc
    res, left = RelocResult(), C.c_int(-7)
    C.memset(C.byref(res), 0xEE, C.sizeof(res))
    rc = L.lvt_amd_reloc_correspond(C.byref(pod), C.byref(cfg), 1, _p(xl), _p(yl), _p(desc_l), None, len(xl), _p(xr), _p(yr), _p(desc_r), len(xr), _p(case["map_xyz"]),
                                    _p(case["map_desc"]), _p(other[0]) if other else None, _p(other[1]) if other else None, len(case["map_xyz"]), case["map_copy"],
                                    case["lost_frame"], C.byref(res), *[_p(a) for a in out], C.byref(left) if claims else None)
    return rc, bytes(res), res, [a.tobytes() for a in out], left.value


def test_reloc_correspond_without_claims_left_and_without_the_other_copy(L):
    """claims_left NULL, and other_pos / other_desc NULL, against the full call that hands in zeros for the other copy, 64 left features against 48 map
    points: the result record and all six output arrays byte for byte"""
    case = RC.scene(64, 48, 7)
    M = len(case["map_xyz"])
    zeros = (np.zeros((M, 3)), np.zeros((M, 32), np.uint8))
    rc, rec, res, arrays, left = _correspond(L, case, zeros, True)
    assert rc == 0 and res.n_corr > 8 and res.n_with_point >= 3 and res.status == -1 and left == 0    # the case forms correspondences, with points
    for other, claims in ((zeros, False), (None, True), (None, False)):
        rc2, rec2, _, arrays2, left2 = _correspond(L, case, other, claims)
        assert rc2 == rc and rec2 == rec and arrays2 == arrays and left2 == (0 if claims else -7), (other is None, claims)


# ---- n = 0 with NULL data pointers: what include/lvt_amd_ext.h says ---------------------------------------------------------------------------------------
def test_pose_info_eval_without_points(L):
    pod = lvt_amd.kitti_params().to_pod()
    rec = lvt_amd.PoseInfo()
    assert L.lvt_amd_pose_info_eval(C.byref(pod), _p(np.array([1.0, 0, 0, 0])), _p(np.zeros(3)), None, None, 0, C.byref(rec)) == 0


def test_reloc_solve_without_correspondences(L):
    """fewer than 3 correspondences with a camera-frame point: status 1, the call returns 1, the pose is zero"""
    z = np.zeros((0, 3))
    rc, _, res, counts, inl, hR, ht = _solve(L, lvt_amd.kitti_params(), z, np.zeros((0, 2), np.float32), z, np.zeros(0, np.uint8), RelocConfig())
    assert rc == 1 and res.status == 1 and res.n_corr == 0 and res.n_with_point == 0
    assert not res.q.any() and not res.p.any() and not res.R.any() and not res.t.any()
    assert (hR == -7.0).all() and (ht == -7.0).all() and (inl == -7).all()                         # written for status 0 and 3 only


def test_reloc_match_device_without_queries_and_without_a_map(L):
    import torch
    q = torch.randint(0, 256, (4, 32), dtype=torch.uint8, device="cuda")
    out = torch.full((4, 4), -77, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert L.lvt_amd_reloc_match_device(None, 0, None, 0, None, None) == 0.0                         # n_query = 0: nothing to do, NULL pointers are fine
    assert L.lvt_amd_reloc_match_device(ptr(q), 0, ptr(q), 4, ptr(out), None) == 0.0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -77).all()                                                        # ... and nothing is written
    assert L.lvt_amd_reloc_match_device(ptr(q), 4, None, 0, ptr(out), None) >= 0.0                   # an empty map: every row is the "absent" record
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == [[-1, INT_MAX, -1, INT_MAX]] * 4


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_their_sentences(L):
    import torch
    q = torch.zeros((8, 32), dtype=torch.uint8, device="cuda")
    out = torch.full((4, 4), -77, dtype=torch.int32, device="cuda")
    assert L.lvt_amd_reloc_match_device(C.c_void_p(q.data_ptr() + 8), 4, C.c_void_p(q.data_ptr()), 4, C.c_void_p(out.data_ptr()), None) < 0
    assert _last(L) == ("lvt_amd_reloc_match_device: n_query must be 0 ... 4096, n_map 0 ... 32768, the pointers device pointers aligned to 16 bytes "
                        "(nothing was changed)")
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -77).all()

    prm = lvt_amd.kitti_params()
    n = 4097
    rc, rec = _solve(L, prm, np.zeros((n, 3)), np.zeros((n, 2), np.float32), np.zeros((n, 3)), np.ones(n, np.uint8), RelocConfig())[:2]
    assert rc == -1 and rec == b"\xEE" * C.sizeof(RelocResult)
    assert _last(L) == "lvt_amd_reloc_solve: a NULL argument, or n outside 0 ... 4096 (nothing was changed)"

    case = RC.scene(64, 48, 7)
    import dataclasses
    rc, rec, _, arrays, _ = _correspond(L, case, None, True, prm=dataclasses.replace(case["prm"], img_height=0))
    assert rc == -1 and rec == b"\xEE" * C.sizeof(RelocResult) and arrays[0] == np.full(lvt_amd.RELOC_CAPACITY, -77, np.int32).tobytes()
    assert _last(L) == "lvt_amd_reloc_correspond: parameters lvt_amd_create would refuse (nothing was changed)"


def test_stages_that_read_no_image_size_accept_a_missing_one(L):
    """lvt_amd_pnp and lvt_amd_pose_info_eval with img_height = 0: the answer of the call with the height given"""
    import dataclasses
    prm, X, uv, q0, p0 = pnp_edge_case("kitti", 16)
    answers = []
    for p in (prm, dataclasses.replace(prm, img_height=0)):
        pod = p.to_pod()
        q = np.zeros(4); t = np.zeros(3); calls = C.c_int(0)
        inl = L.lvt_amd_pnp(C.byref(pod), _p(q0), _p(p0), _p(X), _p(uv), 16, _p(q), _p(t), C.byref(calls))
        rec = lvt_amd.PoseInfo()
        assert L.lvt_amd_pose_info_eval(C.byref(pod), _p(q), _p(t), _p(X), _p(uv), 16, C.byref(rec)) == 0
        answers.append((inl, calls.value, q.tobytes(), t.tobytes(), bytes(rec)))
    assert answers[0][0] > 0 and answers[1] == answers[0]


def test_pnp_trace_refuses_null_parameters(L):
    """(a library from before the stage entries shared one parameter path dereferenced the pointer)"""
    prm, X, uv, q0, p0 = pnp_edge_case("kitti", 16)
    q = np.full(4, -7.0); p = np.full(3, -7.0)
    assert L.lvt_amd_pnp_trace(None, _p(q0), _p(p0), _p(X), _p(uv), 16, _p(q), _p(p), None, None, None, None, None, 0, None) == -1
    assert (q == -7.0).all() and (p == -7.0).all()
