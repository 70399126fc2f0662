"""The float64 model of the implicit viscosity solve (tests/viscosity_model.py) against the properties the solve relies on, on the
small dam break with its tank and on an 8x8x8 block without walls: the assembled matrix is symmetric, its smallest eigenvalue is 1,
CG from u0 = b converges within the stated counts and agrees with a direct solve, momentum is kept without wall friction, the kinetic
energy does not grow, and a uniform translation is left alone in zero iterations."""
import numpy as np
import pytest
import scipy.sparse.linalg as spl

from tests import dfsph_model, viscosity_model as vm
from tests.common import small_dam_break
from tests.oracle_lib import IISPH


# CG iterations to tol = 1e-8 on random velocities (DESIGN.md "Implicit viscosity"), plus two
COUNTS = {0.01: 3 + 2, 1.0: 12 + 2, 100.0: 65 + 2}


def _scenes():
    p, sc = small_dam_break((12, 10, 9), solver=IISPH, double=True)
    p["timestep"] = 1e-3
    yield "dam", p, sc["pos"], sc["bi"][:, :3], sc["vbi"]
    p2, sc2 = small_dam_break((8, 8, 8), solver=IISPH, double=True)   # the same lattice, and no tank
    p2["timestep"] = 1e-3
    yield "block", p2, sc2["pos"], None, None


@pytest.fixture(scope="module")
def scenes():
    out = []
    for name, p, pos, bpos, vb in _scenes():
        rho = dfsph_model.density(p, pos, bpos, vb)
        pairs = dfsph_model.Pairs(p, pos, bpos, vb)
        b = np.random.default_rng(11).normal(size=(len(pos), 3))
        out.append((name, p, pos, bpos, vb, rho, pairs, b))
    return out


def _op(sc, nu, nu_b=0.0):
    name, p, pos, bpos, vb, rho, pairs, b = sc
    return vm.Operator(p, pos, rho, nu, nu_b if bpos is not None else 0.0, bpos, vb, pairs=pairs)


@pytest.mark.parametrize("nu,nu_b", [(0.01, 0.0), (1.0, 0.0), (1.0, 1.0), (100.0, 0.0)])
def test_matrix_is_symmetric_positive_definite_and_matches_apply(scenes, nu, nu_b):
    for sc in scenes:
        op = _op(sc, nu, nu_b)
        M = op.matrix()
        b = sc[-1]
        assert np.max(np.abs(M @ b.reshape(-1) - op.apply(b).reshape(-1))) <= 1e-10 * np.max(np.abs(b)) * abs(M).max()
        asym = abs(M - M.T).max()
        assert asym <= 1e-8 * abs(M).max(), (sc[0], asym)
        S = (M + M.T) * 0.5
        lo = spl.eigsh(S, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0]
        assert lo >= 1 - 1e-9, (sc[0], lo)


@pytest.mark.parametrize("nu", [0.01, 1.0, 100.0])
def test_cg_converges_within_the_stated_counts_and_matches_a_direct_solve(scenes, nu):
    for sc in scenes:
        op, b = _op(sc, nu), sc[-1]
        got = vm.cg(op, b, tol=1e-8, min_iters=1)
        assert got["iters"] == got["queued"] <= COUNTS[nu], (sc[0], got["iters"])
        assert got["residual"] <= 1e-8 * got["rhs_norm"]
        want = spl.spsolve(op.matrix().tocsc(), b.reshape(-1)).reshape(-1, 3)
        assert np.linalg.norm(got["u"] - want) <= 1e-7 * np.linalg.norm(b), sc[0]
        # momentum is kept without wall friction; the kinetic energy does not grow
        assert np.max(np.abs(np.sum(got["u"] - b, axis=0))) <= 1e-10 * np.sum(np.abs(b)), sc[0]
        assert np.sum(got["u"] ** 2) <= np.sum(b ** 2)


def test_wall_friction_takes_energy(scenes):
    sc = scenes[0]
    b = sc[-1]
    slip = vm.cg(_op(sc, 1.0), b, tol=1e-8, min_iters=1)
    stick = vm.cg(_op(sc, 1.0, 1.0), b, tol=1e-8, min_iters=1)
    assert stick["residual"] <= 1e-8 * stick["rhs_norm"]
    assert np.sum(stick["u"] ** 2) < np.sum(slip["u"] ** 2) <= np.sum(b ** 2)


@pytest.mark.parametrize("tol,min_iters", [(1e-8, 0), (1e-8, 2), (0.0, 3)])
def test_uniform_translation_is_left_alone(scenes, tol, min_iters):
    for sc in scenes:
        op = _op(sc, 1.0)
        b = np.tile(np.array([0.3, -1.25, 2.0]), (op.n, 1))
        got = vm.cg(op, b, tol=tol, min_iters=min_iters)
        assert got["iters"] == 0 and got["residual"] == 0.0
        np.testing.assert_array_equal(got["u"], b)


def test_guards():
    assert vm.alpha_of(2.0, 4.0) == 0.5 and vm.alpha_of(2.0, 0.0) == 0.0 and vm.alpha_of(2.0, -1.0) == 0.0
    assert vm.alpha_of(2.0, float("nan")) == 0.0
    assert vm.beta_of(1.0, 4.0) == 0.25 and vm.beta_of(1.0, 0.0) == 0.0
