"""Unregistered depth, CPU tier: the numpy restatement of the registration (tests/depth_reg_util.py) held to its definition -- the identity camera, a
constructed case with the expected plane written out by hand -- and the two 320 x 240 sequences of the GPU tests held to the oracle, which is fed the
numpy-registered planes.  No GPU, no HIP library."""
import numpy as np
import pytest

import lvt_amd
import depth_reg_util as D

F = np.float32


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_identity_camera_returns_the_input_bit_for_bit():
    """K_d = K_c, R = I, t = 0, no distortion, equal sizes: every footprint is its own pixel; the output is the input with +inf where the input is <= 0"""
    prm = lvt_amd.tum_params(width=80, height=60, fx=100.25, fy=100.25, cx=39.3, cy=29.7)
    rng = np.random.default_rng(5)
    d = rng.uniform(0.2, 6.0, (60, 80)).astype(F)
    d[rng.random((60, 80)) < 0.1] = 0.0
    d[3, 4], d[7, 9] = -1.0, np.nan
    reg, span = D.register_numpy(D.identity_camera(prm), prm, d)
    want = np.where(d > 0, d, F(np.inf)).astype(F)
    assert span == (1, 1), span
    assert _same_bits(reg, want)
    # ... and a 16-bit plane registers like its fp32 conversion, padding of a wider destination stays +inf
    u = np.clip(np.rint(np.nan_to_num(d).astype(np.float64) * 5000), 0, 65535).astype(np.uint16)
    s = F(1) / F(5000)
    reg16 = D.register(D.identity_camera(prm), prm, u, s, pitch=96)
    f = u.astype(F) * s
    assert _same_bits(reg16[:, :80], np.where(f > 0, f, F(np.inf)).astype(F)) and np.all(np.isposinf(reg16[:, 80:]))


@pytest.mark.parametrize("name", ["invalid depths", "nearer wins", "behind the camera", "edges"])
def test_constructed_case(name):
    """8 x 6: z = 0 / NaN / -1 / +inf leave no trace; of two depth pixels on one colour pixel the nearer wins; Zc <= 0 behind a 180-degree extrinsic; footprints cut
    by each image edge and one wholly outside -- each against a plane written out by hand"""
    cases, prm = D.constructed_case()
    cam, d, want = cases[name]
    reg = D.register(cam, prm, d)
    assert _same_bits(reg, want), (reg, want)


@pytest.mark.parametrize("axis", [0, 1])
def test_footprint_cap(axis):
    """x1 - x0 = 15 (sixteen pixels) is kept, x1 - x0 = 16 is skipped; rows alike"""
    for diff in (15, 16):
        cam, prm, d, want = D.span_case(diff, axis)
        reg, span = D.register_numpy(cam, prm, d)
        assert _same_bits(reg, want), (diff, np.argwhere(np.isfinite(reg)))
        assert span == ((16, 1) if axis == 0 else (1, 16)) if diff == 15 else span == (0, 0)


@pytest.mark.parametrize("which,limit_px", [("same", 3), ("half", 4)])
def test_oracle_tracks_the_registered_sequences(oracle_lib, which, limit_px):
    """the inputs of the GPU tests: a depth camera 5 cm to the side (focal x 0.9, principal point shifted), at the colour size and at half of it; the oracle fed
    the numpy-registered planes stays TRACKING on all 12 frames, holes <= 10 %, close to the run on the true colour-frame depth (measured: holes 0.01 - 0.03 % --
    with focal x 0.9 a depth pixel covers 1.1 colour pixels, what remains are occlusion shadows --, 283 - 307 features, 266 - 296 matches, position within 0.7 mm.
    The figures are this world's: four fronto-parallel layers whose farthest fills the image, so the sensor has depth everywhere and what stays empty are the
    shadows behind the nearer layers' edges, seen from 5 cm to the side.  A hole rate is a property of the scene: the same camera on the 640 x 480 world, whose
    patches of near layer are half as large in metres and show more edges, leaves 1.6 % of frame 0 empty under this same numpy restatement, and
    profiles/depth_registration.md reports 2.4 % for the last frame of its run.  The bound here is the guard on these inputs)"""
    q, plain = D.sequence(which), D.sequence("plain")
    orc, ref = oracle_lib.Oracle(q.prm, 2), oracle_lib.Oracle(plain.prm, 2)
    for i in range(q.n):
        assert np.array_equal(q.gray[i], plain.gray[i])
        R, t = orc.track_rgbd(q.gray[i], q.f32[i])
        R0, t0 = ref.track_rgbd(plain.gray[i], plain.f32[i])
        c = orc.counts()
        print(f"{which} frame {i}: holes {100 * q.holes[i]:.2f} % n_left {c['n_left']} matches {c['n_matches']} |dt| {1e3 * np.linalg.norm(t - t0):.2f} mm")
        assert orc.status == 2, f"frame {i}: the oracle is not TRACKING"
        assert q.holes[i] <= 0.10, f"frame {i}: {100 * q.holes[i]:.1f} % holes"
        assert np.linalg.norm(t - t0) < 0.01, f"frame {i}: {np.linalg.norm(t - t0)} m from the run on registered depth"
    reg, span = D.register_numpy(q.cam, q.prm, q.s_u16[0], D.SCALE)
    assert max(span) <= limit_px, span
