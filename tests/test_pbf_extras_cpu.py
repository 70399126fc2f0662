"""The PBF tensile correction and vorticity confinement without a GPU: the ABI declares them, and the float64 model
(tests/pbf_extras_model.py) shows the physics the definitions promise: the vorticity of a rigid rotation, the angular momentum that
confinement adds to a rotating block, and the pair that s_corr pushes apart where the clamped constraint does nothing."""
import os
import re

import numpy as np
import pytest

from nereus_amd import capi
from tests import pbf_extras_model as M
from tests.oracle_lib import IISPH, Oracle
from tests.pcisph_model import w_dens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_tensile_and_vorticity():
    text = open(os.path.join(ROOT, "include", "nereus_hip.h")).read()
    assert re.search(r"\bint\s+nrs_pbf_set_tensile\s*\(\s*nrs_ctx\s*\*\s*\w+\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*\)", text)
    assert re.search(r"\bint\s+nrs_pbf_set_vorticity\s*\(\s*nrs_ctx\s*\*\s*\w+\s*,\s*double\s+\w+\s*\)", text)
    assert re.search(r"\bNRS_ARR_VORTICITY\s*=\s*31\b", text)
    for name in ("nrs_pbf_set_tensile", "nrs_pbf_set_vorticity"):
        assert name in capi.EXPORTS
    assert capi.ARRAYS["vorticity"] == (31, "v4")
    assert hasattr(capi.Solver, "pbf_set_tensile") and hasattr(capi.Solver, "pbf_set_vorticity")


def _lattice(nx, ny, nz, s):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)
    return g.astype(np.float64) * s, g


def _params():
    p = Oracle.default_params(IISPH, True)
    m, rd, h = (float(p[k][0]) for k in ("particleMass", "restDensity", "interactionRadius"))
    return p, m, rd, h


@pytest.mark.parametrize("omega", [(0.0, 0.0, 2.0), (0.3, -0.5, 1.0)])
def test_model_vorticity_of_rigid_rotation_is_parallel_to_omega(omega):
    """u = Omega x r on a cubic lattice: at an interior particle omega = c Omega with c > 0 (sum over a cubic shell of d d^T is a
    multiple of the identity)."""
    p, m, rd, h = _params()
    s = 0.7 * h
    x, g = _lattice(7, 7, 7, s)
    Om = np.array(omega)
    u = np.cross(Om, x - x.mean(axis=0))
    ii, jj = M.pairs(p, x)
    w = M.vorticity(p, x, u, ii, jj)
    i = int(np.nonzero(np.all(g == 3, axis=1))[0][0])
    c = float(w[i] @ Om) / float(Om @ Om)
    assert c > 0
    np.testing.assert_allclose(w[i], c * Om, rtol=0, atol=1e-12 * np.linalg.norm(w[i]))


def test_model_confinement_raises_angular_momentum_of_rotating_block():
    """One confinement step on a block in rigid rotation about z: L . Omega grows.  On the side faces N points inward, so N x omega
    points along the motion; on the top and bottom faces, and inside, N x omega is 0."""
    p, m, rd, h = _params()
    dt = float(p["timestep"][0])
    s = float(np.cbrt(m / rd))
    x, g = _lattice(10, 10, 10, s)
    c = x.mean(axis=0)
    Om = np.array([0.0, 0.0, 3.0])
    u = np.cross(Om, x - c)
    ii, jj = M.pairs(p, x)
    w = M.vorticity(p, x, u, ii, jj)
    eta, N = M.confinement(p, x, w, ii, jj)
    kick = np.cross(N, w)
    vel = u + dt * 1.0 * kick

    def lz(v):
        return float(np.sum(m * np.cross(x - c, v)[:, 2]))
    assert lz(vel) > lz(u) * (1 + 1e-9)
    face = lambda a, k: g[:, a] == k   # noqa: E731
    inner = lambda a: np.all([(g[:, b] >= 2) & (g[:, b] <= 7) for b in range(3) if b != a], axis=0)   # noqa: E731
    interior = np.all((g >= 2) & (g <= 7), axis=1)
    assert np.all(kick[interior] == 0)   # |omega| uniform: eta is roundoff, under the cut
    side = (face(0, 0) | face(0, 9)) & inner(0)
    r = (x - c)[side]
    assert np.all(np.sum(N[side][:, :2] * r[:, :2], axis=1) < 0)   # inward
    along = np.sum(kick[side] * np.cross(Om, x[side] - c), axis=1)
    assert np.all(along > 0)
    top = (face(2, 0) | face(2, 9)) & inner(2)
    assert np.max(np.abs(kick[top])) <= 1e-9 * np.max(np.abs(kick[side]))


def test_model_tensile_correction_separates_an_isolated_pair():
    """Two fluid particles at rest 0.8 h apart: m (W(0) + W(0.8 h)) is below rho0, so C = 0 and lambda = 0.  Without s_corr nothing
    moves; with k > 0 the pair separates along its axis."""
    p, m, rd, h = _params()
    kp = float(p["kpoly"][0])
    rho = m * (w_dens(np.zeros((1, 3)), h, kp)[0] + w_dens(np.array([[0.8 * h, 0, 0]]), h, kp)[0])
    assert rho < rd and 0.78 < rho / rd < 0.86
    x = np.array([[0.1, 0.1, 0.1], [0.1 + 0.8 * h, 0.1, 0.1]])
    r0 = M.run(p, x, np.zeros_like(x), min_iters=2, eta=0.0)
    assert np.all(r0["lam"] == 0) and np.array_equal(r0["xs"], x)
    r = M.run(p, x, np.zeros_like(x), min_iters=2, eta=0.0, k=1e-3, dq=0.7)
    assert np.all(r["lam"] == 0)
    d = r["xs"] - x
    assert d[0, 0] < -1e-4 and d[1, 0] > 1e-4   # far above fp32 resolution at |x| ~ 0.1
    np.testing.assert_allclose(d[0], -d[1], rtol=1e-12)
    assert np.all(d[:, 1:] == 0)


def test_model_defaults_equal_pbf_model():
    """k = 0 and eps_v = 0 reproduce tests/pbf_model.py exactly."""
    from tests import pbf_model
    from tests.common import compressed_block
    p, pos, vel = compressed_block(double=True)
    a = pbf_model.run(p, pos, np.zeros_like(pos), min_iters=3, eta=0.0, xsph=0.1)
    b = M.run(p, pos, np.zeros_like(pos), min_iters=3, eta=0.0, xsph=0.1)
    for k in ("lam", "rho", "xs", "vel"):
        np.testing.assert_array_equal(a[k], b[k])
