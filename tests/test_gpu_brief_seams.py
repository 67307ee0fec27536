"""BRIEF at every seam of the `inside` predicates of k_brief and k_brief_img (k_features.hip: two loops over one skeleton -- brief_plane_of_block,
brief_key_points_of_wave, brief_centre, last_block_publishes), frame by frame
against the oracle: case_tables.py, "BRIEF at every seam of `inside`" has the corner list and what each corner is there for; test_case_tables.py holds the
list to its counts with the oracle alone.  Both kernels (LVT_AMD_BRIEF_FROM_IMAGE unset / 1), as a single handle (the sequence by value) and as two seats
of one lock-step pool (the sequence from the device array, each plane's sequence picked by the kernel itself)."""
import gc
import threading

import numpy as np
import pytest

from case_tables import BRIEF_SEAM_FRAMES, brief_seam_case, brief_seam_expected, brief_seam_tally
from parity_util import POSE_TOL, diff_frame, pose_errors

pytestmark = pytest.mark.gpu


def _run(hip, orc, frames, fails):
    """the frames through one handle and its oracle: the full diff, the pose, and the survivors of the border filter (count and order) on every frame"""
    keep_l, keep_r = brief_seam_expected(frames[0][2])[0], brief_seam_expected(frames[0][3])[0]
    for i, f in enumerate(frames):
        Ro, to = orc.track_with_external_corners(*f)
        Rh, th = hip.track_with_external_corners(*f)
        msgs = diff_frame(hip, orc)
        e_t, e_R = pose_errors(Rh, th, Ro, to)
        if e_t > POSE_TOL or e_R > POSE_TOL:
            msgs.append(f"pose e_t={e_t:.3e} e_R={e_R:.3e}")
        c = hip.counts()
        if (c["n_left"], c["n_right"]) != (int(keep_l.sum()), int(keep_r.sum())):
            msgs.append(f"kept corners {c['n_left']} / {c['n_right']}")
        if not np.array_equal(hip.features(0)[0], f[2].astype(np.float32)[keep_l]) or not np.array_equal(hip.features(1)[0], f[3].astype(np.float32)[keep_r]):
            msgs.append("the kept corners are not the expected ones in list order")
        if hip.get_state() != 2 or orc.status != 2:
            msgs.append(f"status {hip.get_state()} / {orc.status}")
        if msgs:
            fails.append((i, msgs[:5]))
            return


@pytest.mark.parametrize("seats", [1, 2], ids=["single_handle", "pool_of_two"])
@pytest.mark.parametrize("from_image", [None, "1"], ids=["k_brief", "k_brief_img"])
def test_brief_at_the_seams_of_inside(hip_lib, oracle_lib, monkeypatch, from_image, seats):
    """58 of the 65 listed corners survive brief_border_keep in either eye (test_case_tables.py derives the number); 15 of the left eye's and 8 of the
    right eye's take k_brief_img's clipped element-wise path -- four below the last row its patch fits, the others on the four columns where the patch's
    64 columns would overrun a row pitch equal to the width -- and all of them k_brief's window path.  Descriptors, hence every later stage, are the oracle's."""
    from oracle import pyoracle as O
    if from_image is None:
        monkeypatch.delenv("LVT_AMD_BRIEF_FROM_IMAGE", raising=False)
    else:
        monkeypatch.setenv("LVT_AMD_BRIEF_FROM_IMAGE", from_image)
    prm, frames = brief_seam_case()
    tally = brief_seam_tally(frames[0][2])
    assert len(frames) == BRIEF_SEAM_FRAMES and tally["kept"] == 58 and tally["slow_img"] == 15 and tally["slow_plane"] == 0
    gc.collect()        # (seats share their pool's parameters: a forgotten seat of an earlier test must be gone before these found a pool of their own)
    hs = [hip_lib.LvtSystem.create(prm, 1, pooled=(seats > 1)) for _ in range(seats)]
    assert seats == 1 or all(h.ordering() == "pooled" for h in hs)
    orcs = [O.Oracle(prm, 1) for _ in range(seats)]
    fails = [[] for _ in range(seats)]
    ths = [threading.Thread(target=_run, args=(hs[k], orcs[k], frames, fails[k])) for k in range(seats)]
    for t in ths: t.start()
    for t in ths: t.join()
    errors = [h.last_error() for h in hs]
    for h in hs: h.close()
    assert fails == [[] for _ in range(seats)], fails
    assert errors == [""] * seats, errors
