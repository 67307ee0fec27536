"""-m gpu: relocalisation's correspondence stage (stage 2 of include/lvt_amd_ext.h, RELOCALISATION) through its stage entry lvt_amd_reloc_correspond -- the
launches of a handle's call: k_reloc_match, k_reloc_corr, k_reloc_points, k_reloc_list -- against tests/reloc_util.py on the planted cases of
tests/reloc_cases.py.  Everything is compared bit for bit: the counts and indices are integers, X and (u, v) are copies, and Pc is fp64 with one IEEE
operation per written operation, so equality is the claim and no tolerance enters.  What the call must not write -- elements beyond the counts, Pc where
has_pc is 0 -- must come back as the sentinels the wrapper put there.  Two more tests tie the entry to a handle's own call."""
import numpy as np
import pytest

import lvt_amd
import reloc_cases
import reloc_util as RU

pytestmark = pytest.mark.gpu

COUNTS = ("n_features", "n_map", "n_matched", "n_corr", "n_with_point", "status")


def _run(hip_lib, case):
    return hip_lib.reloc_correspond(case["prm"], case["sensor"], case["xy_l"], case["desc_l"], case["map_xyz"], case["map_desc"], right=case["right"],
                                    depth=case["depth"], other=case["other"], map_copy=case["map_copy"], lost_frame=case["lost_frame"],
                                    cfg=lvt_amd.RelocConfig(min_disparity=case["min_disparity"]))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1) if len(a) else np.zeros((0, 0), np.uint8)


def hold(got, ref, tag):
    """every output of the entry against the restatement, and the sentinels where nothing may be written"""
    print(tag, {k: got[k] for k in COUNTS}, "ref", {k: ref[k] for k in COUNTS}, "claims left", got["claims_left"])
    assert {k: got[k] for k in COUNTS} == {k: ref[k] for k in COUNTS}, tag
    n, n3 = ref["n_corr"], ref["n_with_point"]
    assert np.array_equal(got["feat"][:n], ref["feat"]), (tag, np.flatnonzero(got["feat"][:n] != ref["feat"])[:5])
    assert np.array_equal(_bits(got["X"][:n]), _bits(ref["X"])), tag
    assert np.array_equal(_bits(got["uv"][:n]), _bits(np.asarray(ref["uv"], np.float32))), tag
    assert np.array_equal(got["has_pc"][:n], ref["has_pc"].astype(np.uint8)), (tag, np.flatnonzero(got["has_pc"][:n] != ref["has_pc"])[:5])
    has = ref["has_pc"].astype(bool)
    bad = np.flatnonzero((_bits(got["pc"][:n][has]) != _bits(ref["pc"][has])).any(axis=1))
    assert bad.size == 0, (tag, bad[:5], got["pc"][:n][has][bad[:2]], ref["pc"][has][bad[:2]])
    assert np.array_equal(got["with_pc"][:n3], ref["with_pc"]), tag
    # nothing beyond the counts, no Pc without a point: the sentinels are intact
    assert (got["feat"][n:] == lvt_amd.RELOC_SENTINEL_INT).all() and (got["with_pc"][n3:] == lvt_amd.RELOC_SENTINEL_INT).all(), tag
    assert (got["X"][n:] == lvt_amd.RELOC_SENTINEL_F64).all() and (got["uv"][n:] == lvt_amd.RELOC_SENTINEL_F32).all(), tag
    assert (got["has_pc"][n:] == lvt_amd.RELOC_SENTINEL_BYTE).all() and (got["pc"][n:] == lvt_amd.RELOC_SENTINEL_F64).all(), tag
    assert (got["pc"][:n][~has] == lvt_amd.RELOC_SENTINEL_F64).all(), tag
    assert got["claims_left"] == 0, tag                       # the claim table is left as it was found


@pytest.mark.parametrize("name", reloc_cases.CASE_NAMES)
def test_correspond_case(hip_lib, name):
    case, ref = reloc_cases.case_and_answer(name)
    hold(_run(hip_lib, case), ref, f"{name} ({case['plants']})")


# ---- the entry and a handle's own call ------------------------------------------------------------------------------------------------------------------------
def _as_case(prm, sys_):
    xyz, _, _, desc = sys_.map()
    (xy, _, de), (xyr, _, der) = sys_.features(0), sys_.features(1)
    return dict(prm=prm, sensor=1, xy_l=xy, desc_l=de, right=(xyr, der), depth=None, other=None, map_xyz=xyz, map_desc=desc, map_copy=0, lost_frame=0, min_disparity=1.0)


def test_entry_returns_what_the_handles_call_counts(hip_lib):
    """a handle TRACKING on the half-size kitti world: the entry, fed the handle's features(0), features(1) and map(), returns the n_matched, n_corr and
    n_with_point of the handle's dry run -- and the restatement's everything"""
    from parity_util import make_case
    world, prm, sensor = make_case("kitti", 0, 0.5)
    sys_ = hip_lib.LvtSystem.create(prm, sensor)
    for i in range(5):
        sys_.track(*world.render_stereo(i))
    assert sys_.get_state() == 2
    case = _as_case(prm, sys_)
    assert len(case["xy_l"]) > 100 and len(case["right"][0]) > 100
    dry = sys_.relocalise(dry_run=1)
    got = _run(hip_lib, case)
    fields = ("n_features", "n_map", "n_matched", "n_corr", "n_with_point")
    print({k: got[k] for k in fields}, {k: getattr(dry, k) for k in fields})
    assert {k: got[k] for k in fields} == {k: getattr(dry, k) for k in fields} and dry.n_corr > 50
    hold(got, reloc_cases.restate(case), "tracking handle")
    sys_.close()


def test_handle_with_more_than_1024_features(hip_lib, oracle_lib):
    """the only handle state with more than 1024 correspondences: two epochs of the noise recipe (lvt_amd.synth.noise_frame: ~4 000 external corners a frame,
    every fresh corner triangulated), a dry run on the TRACKING handle.  The restatement is fed nothing but what the handle returns; every integer field
    equal, the pose within the bounds of the sequence cases of test_gpu_relocalisation.py"""
    from lvt_amd.synth import noise_frame
    from test_gpu_relocalisation import INT_FIELDS
    prm = lvt_amd.kitti_params(width=1241, height=376)
    prm.triangulation_policy, prm.staged_threshold, prm.untracked_threshold = 2, 0, 1000
    sys_ = hip_lib.LvtSystem.create(prm, 1)
    for e in range(2):
        sys_.track_with_external_corners(*noise_frame(e))
    assert sys_.get_state() == 2 and sys_.last_error() == "", sys_.last_error()
    case = _as_case(prm, sys_)
    ref = RU.relocalise(prm, 1, case["map_xyz"], case["map_desc"], case["xy_l"], case["desc_l"], right=case["right"], pnp=oracle_lib.pnp)
    res = sys_.relocalise(dry_run=1)
    print({k: getattr(res, k) for k in INT_FIELDS}, "ref", {k: ref[k] for k in INT_FIELDS})
    assert res.n_features > 3000 and res.n_corr > 1024
    assert {k: getattr(res, k) for k in INT_FIELDS} == {k: ref[k] for k in INT_FIELDS}
    assert np.allclose(res.p, ref["p"], rtol=0, atol=1e-7) and np.allclose(res.q, ref["q"], rtol=0, atol=1e-9), (res.p, ref["p"], res.q, ref["q"])
    hold(_run(hip_lib, case), reloc_cases.restate(case), "noise handle")          # ... and the entry on the same data, output by output
    assert sys_.get_state() == 2
    sys_.close()
