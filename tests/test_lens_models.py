"""The lens models on the CPU: the numpy restatement (tests/lens_util.py) of "LENS MODELS" (include/lvt_amd_ext.h) held to the existing plumb-bob restatement
and to the oracle where they overlap, to entries worked out by hand, to each model's own forward formula, and -- through the oracle's tracker -- to the
claim that worlds rectified through these maps can be tracked at all (the GPU tier's sequence tests compare against exactly these chains)."""
import math

import numpy as np
import pytest

import lens_util as LU
from lens_util import RADTAN, FISHEYE
from remap_util import rectify_maps, maps_equal, remap

EYE3 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


# ---- 1. where the models overlap ------------------------------------------------------------------------------------------------------------
def _euroc():
    from test_oracle_primitives import EUROC_L
    return EUROC_L


@pytest.mark.parametrize("size", [(752, 480), (67, 35)])
def test_radtan_with_seven_zeros_is_the_plumb_bob_restatement(size):
    """RADTAN with k4 ... s4 = 0 and a destination of the source's size: bit for bit remap_util.rectify_maps"""
    c = _euroc()
    w, h = size
    want = rectify_maps(c["K"], c["D"], c["R"], c["P"], w, h)
    got = LU.lens_maps(RADTAN, c["K"], list(c["D"]) + [0.0] * 7, c["R"], c["P"], w, h)
    assert maps_equal(got[0], want[0]) and maps_equal(got[1], want[1])
    short = LU.lens_maps(RADTAN, c["K"], c["D"], c["R"], c["P"], w, h)     # (a shorter D is padded with zeros)
    assert maps_equal(short[0], want[0]) and maps_equal(short[1], want[1])


def test_radtan_with_seven_zeros_is_the_oracles_map(oracle_lib):
    c = _euroc()
    want = oracle_lib.init_undistort_rectify_map(c["K"], c["D"], c["R"], c["P"], 752, 480)
    got = LU.lens_maps(RADTAN, c["K"], list(c["D"]) + [0.0] * 7, c["R"], c["P"], 752, 480)
    assert maps_equal(got[0], want[0]) and maps_equal(got[1], want[1])


# ---- 2. entries worked out by hand ------------------------------------------------------------------------------------------------------------
def test_fisheye_without_distortion_at_the_principal_ray_and_45_degrees_off_axis():
    """P = [[1, 0, 0], [0, 1, 0], [0, 0, 1]] makes destination pixel (j, i) the ray (j, i, 1).  Pixel (0, 0) is the principal ray: r = 0, scale = 1,
    u = u0, v = v0.  Pixel (j, i) with j = i and j^2 + i^2 = 1 would be 45 degrees off axis; on the integer grid the ray (1, 1, 1) has r = sqrt(2),
    and the 45-degree ray is reached with P = diag(sqrt(2), sqrt(2), 1): pixel (1, 1) is the ray (1 / sqrt(2), 1 / sqrt(2), 1), r = 1, theta = pi / 4,
    x = y = 1 / sqrt(2): u - u0 = fx (pi / 4) / sqrt(2)."""
    K = [300.0, 0.0, 20.5, 0.0, 310.0, 11.25, 0.0, 0.0, 1.0]
    u, v = LU.lens_maps_f64(FISHEYE, K, [0.0] * 4, EYE3, EYE3, 3, 3)
    assert u[0, 0] == 20.5 and v[0, 0] == 11.25
    s = math.sqrt(2.0)
    u, v = LU.lens_maps_f64(FISHEYE, K, [0.0] * 4, EYE3, [s, 0.0, 0.0, 0.0, s, 0.0, 0.0, 0.0, 1.0], 3, 3)
    assert u[0, 0] == 20.5 and v[0, 0] == 11.25
    assert abs((u[1, 1] - 20.5) - 300.0 * (math.pi / 4) / s) < 1e-10
    assert abs((v[1, 1] - 11.25) - 310.0 * (math.pi / 4) / s) < 1e-10


def test_radtan_with_only_k4():
    """P = I: pixel (1, 0) is the ray (1, 0, 1): r2 = 1, kr = 1 / (1 + k4), xd = kr, yd = 0.  k4 = 0.25: kr = 0.8 -- u = fx 0.8 + u0, v = v0.  Pixel (1, 2) is
    the ray (1, 2, 1): r2 = 5, kr = 1 / (1 + 5 k4) = 1 / 2.25: u = fx / 2.25 + u0, v = 2 fy / 2.25 + v0."""
    K = [100.0, 0.0, 7.0, 0.0, 200.0, 3.0, 0.0, 0.0, 1.0]
    D = [0.0] * 5 + [0.25] + [0.0] * 6
    u, v = LU.lens_maps_f64(RADTAN, K, D, EYE3, EYE3, 3, 3)
    assert u[0, 1] == 100.0 * (1.0 / 1.25) + 7.0 and v[0, 1] == 3.0
    assert abs(u[2, 1] - (100.0 / 2.25 + 7.0)) < 1e-12 and abs(v[2, 1] - (400.0 / 2.25 + 3.0)) < 1e-12


def test_fisheye_behind_the_camera_is_signed_infinity():
    """R a rotation of 75 degrees about y puts the new camera's horizon inside the image: where _w <= 0 the entries are -inf / +inf by the sign of _x, _y, and
    the remap turns them into pixel 0"""
    K = [30.0, 0.0, 33.2, 0.0, 30.0, 17.4, 0.0, 0.0, 1.0]
    a = math.radians(75.0)
    R = [math.cos(a), 0.0, math.sin(a), 0.0, 1.0, 0.0, -math.sin(a), 0.0, math.cos(a)]
    m1, m2 = LU.lens_maps(FISHEYE, K, [0.0] * 4, R, K, 67, 35)
    n_inf = int(np.sum(np.isinf(m1)))
    print("entries that are +-inf:", n_inf, "of", m1.size)
    assert n_inf == 910 and np.array_equal(np.isinf(m1), np.isinf(m2))
    plane, code = remap(np.full((35, 67), 200, np.uint8), m1, m2)
    assert not plane[np.isinf(m1)].any()


# ---- 3. round trips through each model's forward formula -------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,D", [(RADTAN, [0.12, 0.02, 2e-4, -1e-4, 0.01, 0.05, 0.01, 0.002, 1e-3, -5e-4, 5e-4, 1e-3]),
                                     (FISHEYE, [-0.02, 0.004, -0.001, 0.0002]), (FISHEYE, [0.6, 0.05, 0.0, 0.0])])
def test_round_trip_through_the_forward_formula(model, D):
    """a destination pixel (j, i) is the ray ((j - cx') / fx', (i - cy') / fy', 1) (R = I); that ray through the model's own forward formula lands on the
    raw pixel the map holds at [i, j]: within 1e-9 px in fp64, before the float cast"""
    K = [400.0, 0.0, 201.3, 0.0, 410.0, 98.7, 0.0, 0.0, 1.0]
    P = [300.0, 0.0, 160.2, 0.0, 300.0, 80.9, 0.0, 0.0, 1.0]
    dw, dh = 321, 163
    u, v = LU.lens_maps_f64(model, K, D, EYE3, P, dw, dh)
    worst = 0.0
    for i in range(0, dh, 9):
        for j in range(0, dw, 7):
            pu, pv = LU.project(model, K, D, (j - P[2]) / P[0], (i - P[5]) / P[4])
            worst = max(worst, abs(pu - u[i, j]), abs(pv - v[i, j]))
    print(f"worst round-trip distance {worst:.3e} px")
    assert worst <= 1e-9


# ---- 4. the oracle tracks on worlds rectified through these maps ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fisheye_strong", "fisheye_mild", "radtan12", "fisheye_small"])
def test_the_oracle_tracks_the_rectified_world(oracle_lib, name):
    from lens_cases import get_case
    c = get_case(name)
    m1, m2 = c.numpy_maps()
    outside = LU.outside_fraction(m1, m2, c.sw, c.sh)
    print(f"{name}: {100 * outside:.1f} % of the map entries outside the {c.sw} x {c.sh} source")
    if name == "fisheye_strong":
        assert outside > 0.05       # (a condition on the input: the border branches run)
    if name == "fisheye_small":
        assert c.sw < c.dw and c.sh < c.dh
    orc = oracle_lib.Oracle(c.prm, 1)
    states, matches = [], []
    for L, R in c.rectified():
        orc.track(L, R)
        states.append(orc.status)
        matches.append(orc.counts()["n_matches"])
    print(f"{name}: states {states} matches {matches}")
    assert states == [2] * len(states), f"{name}: the oracle is not TRACKING on every frame: {states}"
