"""Kinematic boundary bodies without a GPU: the float64 model's pose integration, transform and wall velocity (tests/bodies_model.py),
the four entry points in the built library and the binding, and the error codes that need no device."""
import ctypes as C
import os
import re

import numpy as np

from nereus_amd import capi
from tests import bodies_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["nrs_set_boundary_bodies", "nrs_set_body_velocity", "nrs_set_body_pose", "nrs_get_body_pose"]


def test_rotation_stays_orthonormal_over_many_steps():
    x, q = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
    for k in range(2000):
        x, q = bm.advance(x, q, (0.1, 0.0, -0.2), (3.0, -7.0, 11.0), 1e-3 * (1 + (k % 3)))
    R = bm.rotation(q)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14
    assert abs(np.linalg.det(R) - 1.0) < 1e-14
    assert abs(q @ q - 1.0) < 1e-15


def test_n_steps_at_constant_omega_are_one_rotation():
    omega, dt, n = np.array([0.3, -1.2, 2.0]), 2.5e-3, 400
    x, q = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
    for _ in range(n):
        x, q = bm.advance(x, q, (0, 0, 0), omega, dt)
    once = bm.exp_half(omega, n * dt)
    assert np.abs(q - once).max() < 1e-13
    # ... and the rotation matrix is Rodrigues' formula for the angle n dt |omega|
    wn = np.sqrt(omega @ omega)
    a, th = omega / wn, n * dt * wn
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    assert np.abs(bm.rotation(q) - (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K)).max() < 1e-13


def test_zero_omega_leaves_q_untouched_exactly():
    q0 = np.array([0.1, 0.7, -0.3, 0.2])
    q0 = q0 / np.sqrt(q0 @ q0)
    x, q = bm.advance((1.0, 2.0, 3.0), q0, (0.5, 0.0, 0.0), (0.0, 0.0, 0.0), 1e-3)
    assert q is q0
    np.testing.assert_array_equal(x, [1.0005, 2.0, 3.0])


def test_transform_and_wall_velocity():
    rng = np.random.default_rng(3)
    rest = rng.uniform(-1, 1, (9, 3)).astype(np.float32)
    b = bm.Body(rest, v=(0.2, 0.0, 0.1), omega=(0.0, 0.0, 2.0))
    np.testing.assert_array_equal(b.x, b.c)
    p0, bound = b.world(np.float32)
    assert np.all(np.abs(p0 - rest) <= bound)          # identity pose: the rest positions, up to the rounding of c
    for _ in range(50):
        b.step(1e-3)
    p, _ = b.world(np.float64)
    # rigid: pairwise distances are those of the rest pose; the origin moved by 50 dt v
    d0 = np.linalg.norm(rest[:, None] - rest[None], axis=2)
    d1 = np.linalg.norm(p[:, None] - p[None], axis=2)
    assert np.abs(d1 - d0).max() < 1e-6
    assert np.abs(b.x - (b.c + 0.05 * b.v)).max() < 1e-15
    # u_b against a finite difference of the motion
    dt = 1e-6
    b2 = bm.Body(rest, v=b.v, omega=b.omega)
    b2.x, b2.q = bm.advance(b.x, b.q, b.v, b.omega, dt)
    pa, _ = b2.world(np.float64)
    u = bm.wall_velocity(p, b.x, b.v, b.omega)
    assert np.abs((pa - p) / dt - u).max() < 1e-5


def test_library_and_binding_have_the_entry_points():
    lib = capi.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS
    text = open(os.path.join(ROOT, "include", "nereus_hip.h")).read()
    assert re.search(r"NRS_MAX_BODIES\s*=\s*16\b", text) and capi.MAX_BODIES == 16
    assert re.search(r"NRS_ARR_B_BODY\s*=\s*35\b", text) and capi.ARRAYS["b_body"] == (35, "u")
    for name in ("set_boundary_bodies", "set_body_velocity", "set_body_pose", "body_pose"):
        assert callable(getattr(capi.Solver, name))


def test_null_context_is_refused_without_a_device():
    """all a machine without a GPU can ask (nrs_create needs a device): NRS_E_INVALID for a NULL context, from each of the four"""
    lib = capi.load_library()
    v3, q4 = (C.c_double * 3)(), (C.c_double * 4)(1.0)
    ids = (C.c_uint32 * 4)()
    assert lib.nrs_set_boundary_bodies(None, ids, 4, 2) == -1
    assert lib.nrs_set_body_velocity(None, 1, v3, v3) == -1
    assert lib.nrs_set_body_pose(None, 1, v3, q4) == -1
    assert lib.nrs_get_body_pose(None, 1, v3, q4) == -1
    assert b"NULL context" in lib.nrs_last_error()
