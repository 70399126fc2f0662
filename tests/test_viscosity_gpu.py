"""The implicit viscosity solve of the DFSPH step on the device (nrs_dfsph_set_viscosity, DESIGN.md "Implicit viscosity"): against the
float64 model (tests/viscosity_model.py) after 1 and 3 fixed iterations in every build, on both kernel paths, with and without wall
workgroups and on the overflow fallback; converged against a direct solve of the model's matrix; the same bits on both paths, on a
repeat and on a block of more than 1024 workgroups; momentum, energy, a uniform translation and the off switch; inside full steps with
Akinci's surface model and an emitter; the refusals.

The right-hand side b of a case is NRS_ARR_VEL_ADV after nrs_step_partial(P_ADVECT) on a twin context with the solve off, whose
NRS_ARR_FORCES_ADV is byte-equal.  Bars, relative to max |b| (the norms: to |b|_2): 1e-4 in fp32 and 1e-10 in fp64, the project's
DFSPH bars.
"""
import re

import numpy as np
import pytest
import scipy.sparse.linalg as spl

from nereus_amd import capi, scene
from tests import viscosity_model as vm
from tests.common import compressed_block, small_dam_break

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
DFSPH_FIXED = (0.0, 2, 0.0, 1, 0)   # nrs_dfsph_configure: nothing read back, no warm start (a twin follows it exactly)
LIST, LIST_NO_WALL_GROUPS, REF = 0, capi.FLAG_NO_WALL_WORKGROUPS, capi.FLAG_REFERENCE_ORDER
BAR = {False: 1e-4, True: 1e-10}


def _random_vel(pos, seed=3):
    vel = np.zeros_like(pos)
    vel[:, :3] = np.random.default_rng(seed).normal(size=(len(pos), 3)).astype(pos.dtype)
    return vel


def _scene(name, double=False, kernel_set=capi.MULLER):
    """(params, pos, vel, bi, vbi): normal random velocities on the dam break with its tank (1080 particles, 5 workgroups, wall
    workgroups), on the 8x8x8 block of the same lattice without walls, on a block at spacing 0.55 h (26 neighbours inside h: every
    interior hit list overflows its 20 entries), and on a block of 65 x 65 x 64 = 270 400 particles (1057 workgroups)."""
    real = np.float64 if double else np.float32
    if name == "dam":
        p, sc = small_dam_break((12, 10, 9), solver=capi.DFSPH, double=double, kernel_set=kernel_set)
        return p, sc["pos"], _random_vel(sc["pos"]), sc["bi"], sc["vbi"]
    if name == "block":
        p, sc = small_dam_break((8, 8, 8), solver=capi.DFSPH, double=double, kernel_set=kernel_set)
        return p, sc["pos"], _random_vel(sc["pos"]), None, None
    if name == "overflow":
        p, pos, _ = compressed_block((8, 8, 8), solver=capi.DFSPH, double=double, kernel_set=kernel_set, ratio=0.55)
        return p, pos, _random_vel(pos), None, None
    assert name == "big"
    p, _ = small_dam_break((2, 2, 2), solver=capi.DFSPH, double=double, kernel_set=kernel_set)
    pos = scene.fluid_block(65, 65, 64, float(p["interactionRadius"][0]), real=real)
    pos[:, :3] -= real(1.05)   # inside the default grid's window
    return p, pos, _random_vel(pos), None, None


def _ctx(sc, double=False, kernel_set=capi.MULLER, flags=0, visc=None, capacity=None, dfsph=DFSPH_FIXED):
    p, pos, vel, bi, vbi = sc
    s = capi.Solver(p, capacity or len(pos), solver=capi.DFSPH, double=double, kernel_set=kernel_set, flags=flags)
    s.dfsph_configure(*dfsph)
    s.set_particles(pos, vel)
    s.set_boundaries(bi, vbi, update_grid=True)
    if visc is not None:
        s.dfsph_set_viscosity(*visc)
    return s


def _twin(sc, double=False, kernel_set=capi.MULLER, flags=0):
    """the sorted state of the step and b, from a context with the solve off"""
    s = _ctx(sc, double, kernel_set, flags)
    s.step_partial(capi.STAGE_P_ADVECT)
    o = dict(x=s.get("sortedPos"), rho=s.get("dens"), b=s.get("velAdv"), forces=s.get("forcesAdv"), bs=s.get("bSorted") if sc[3] is not None else None)
    s.close()
    return o


def _overflowed(sc, double=False):
    """how many hit lists of the scene's first step overflowed (the statistic is a full step's)"""
    s = _ctx(sc, double)
    s.step(1)
    n = s.get_stat(capi.STAT_HIT_OVERFLOW)
    s.close()
    return n


def _solve(sc, tw, double, kernel_set, flags, visc):
    """vel_adv and the info after P_ADVECT with the solve on; the twin really is a twin"""
    s = _ctx(sc, double, kernel_set, flags, visc)
    s.step_partial(capi.STAGE_P_ADVECT)
    u, info = s.get("velAdv"), s.dfsph_viscosity_info()
    assert s.get("forcesAdv").tobytes() == tw["forces"].tobytes()
    assert u[:, 3].tobytes() == tw["b"][:, 3].tobytes()
    s.close()
    return u, info


def _operator(sc, tw, nu, nu_b, kernel_set=capi.MULLER):
    bs = tw["bs"]
    return vm.Operator(sc[0], tw["x"], tw["rho"], nu, nu_b, None if bs is None else bs[:, :3], None if bs is None else bs[:, 3], kernel_set)


def _paths(name, kernel_set):
    if kernel_set != capi.MULLER:
        return [REF, LIST]   # (a Monaghan build has no list kernels: both take the reference-order launch)
    return [LIST, REF] + ([LIST_NO_WALL_GROUPS] if name == "dam" else [])


# ---- 1. against the model, fixed mode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("kernel_set", [capi.MULLER, capi.MONAGHAN], ids=["muller", "monaghan"])
@pytest.mark.parametrize("name", ["dam", "block", "overflow"])
def test_fixed_iterations_match_the_model(hip_lib, name, kernel_set, double):
    sc = _scene(name, double, kernel_set)
    tw = _twin(sc, double, kernel_set)
    if name == "overflow" and kernel_set == capi.MULLER:
        assert _overflowed(sc, double) > 0   # the walk_cells fallback really runs
    b = tw["b"][:, :3].astype(np.float64)
    scale, norm = np.max(np.abs(b)), np.linalg.norm(b)
    bar = BAR[double]
    for nu in (0.01, 1.0):
        for nu_b in ((0.0, 1.0) if sc[3] is not None else (0.0,)):
            op = _operator(sc, tw, nu, nu_b, kernel_set)
            for iters in (1, 3):
                want = vm.cg(op, b, tol=0.0, min_iters=iters)
                for flags in _paths(name, kernel_set):
                    u, info = _solve(sc, tw, double, kernel_set, flags, (nu, nu_b, 0.0, iters, 0))
                    what = (name, nu, nu_b, iters, flags)
                    err = np.max(np.abs(u[:, :3] - want["u"])) / scale
                    eres, erhs = abs(info["residual"] - want["residual"]) / norm, abs(info["rhs_norm"] - want["rhs_norm"]) / norm
                    print("visc-fixed", what, "err %.3e residual %.3e rhs %.3e" % (err, eres, erhs))
                    assert info["on"] and info["iterations"] == want["iters"] == iters, (what, info)
                    assert err <= bar and eres <= bar and erhs <= bar, (what, err, eres, erhs)


# ---- 2. converged ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,tol", [(True, 1e-8), (False, 1e-4)], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["dam", "block"])
def test_converged_matches_a_direct_solve(hip_lib, name, double, tol):
    sc = _scene(name, double)
    tw = _twin(sc, double)
    b = tw["b"][:, :3].astype(np.float64)
    for nu, nu_b in ((1.0, 0.0), (1.0, 1.0)) if name == "dam" else ((0.01, 0.0), (1.0, 0.0)):
        op = _operator(sc, tw, nu, nu_b)
        want = spl.spsolve(op.matrix().tocsc(), b.reshape(-1)).reshape(-1, 3)
        model = vm.cg(op, b, tol=tol, min_iters=1)
        u, info = _solve(sc, tw, double, capi.MULLER, LIST, (nu, nu_b, tol, 1, 0))
        err = np.linalg.norm(u[:, :3] - want) / np.linalg.norm(b)
        print("visc-converged", name, nu, nu_b, "err %.3e iterations %d model %d residual %.3e" % (err, info["iterations"], model["iters"],
                                                                                                 info["residual"] / info["rhs_norm"]))
        assert err <= 10 * tol, (name, nu, nu_b, err)
        assert info["iterations"] == model["iters"], (name, nu, nu_b, info, model["iters"])
        assert info["residual"] <= tol * info["rhs_norm"]


# ---- 3. the same bits -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dam", "block", "overflow"])
def test_both_paths_and_a_repeat_give_the_same_bits(hip_lib, name):
    sc = _scene(name)
    tw = _twin(sc)
    if name == "overflow":
        assert _overflowed(sc) > 0
    for visc in ((1.0, 1.0 if name == "dam" else 0.0, 0.0, 3, 0), (1.0, 0.0, 1e-4, 1, 0)):
        got = [_solve(sc, tw, False, capi.MULLER, flags, visc) for flags in (LIST, REF, LIST, LIST_NO_WALL_GROUPS)]
        for u, info in got[1:]:
            assert u.tobytes() == got[0][0].tobytes(), (name, visc)
            assert info == got[0][1]
        assert got[0][0].tobytes() != tw["b"].tobytes()


def test_big_block_repeats_bit_for_bit(hip_lib):
    """more than 1024 workgroups: the reductions' strided path"""
    sc = _scene("big")
    assert (len(sc[1]) + 255) // 256 > 1024
    tw = _twin(sc)
    got = [_solve(sc, tw, False, capi.MULLER, LIST, (1.0, 0.0, 0.0, 3, 0)) for _ in range(2)]
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1] == got[1][1]
    b, u = tw["b"][:, :3].astype(np.float64), got[0][0][:, :3].astype(np.float64)
    assert np.isfinite(u).all() and got[0][1]["iterations"] == 3
    assert abs(got[0][1]["rhs_norm"] - np.linalg.norm(b)) <= 1e-6 * np.linalg.norm(b)
    assert np.max(np.abs(np.sum(u - b, axis=0))) <= 1e-5 * np.sum(np.abs(b))
    assert np.sum(u * u) <= np.sum(b * b) * (1 + 1e-6)


# ---- 4. invariants on the device --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,mom", [(False, 1e-5), (True, 1e-12)], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["dam", "block"])
def test_momentum_and_energy(hip_lib, name, double, mom):
    sc = _scene(name, double)
    tw = _twin(sc, double)
    b = tw["b"][:, :3].astype(np.float64)
    for visc in ((1.0, 0.0, 0.0, 3, 0), (100.0, 0.0, 1e-3 if not double else 1e-8, 1, 0), (0.01, 0.0, 0.0, 1, 0)):
        u = _solve(sc, tw, double, capi.MULLER, LIST, visc)[0][:, :3].astype(np.float64)
        dm = np.max(np.abs(np.sum(u - b, axis=0))) / np.sum(np.abs(b))
        print("visc-momentum", name, double, visc, "%.3e" % dm, "energy %.6f" % (np.sum(u * u) / np.sum(b * b)))
        assert dm <= mom, (name, visc, dm)
        assert np.sum(u * u) <= np.sum(b * b) * (1 + 1e-6)
    if name == "dam":   # wall friction only takes energy
        u = _solve(sc, tw, double, capi.MULLER, LIST, (1.0, 1.0, 0.0, 3, 0))[0][:, :3].astype(np.float64)
        assert np.sum(u * u) <= np.sum(b * b) * (1 + 1e-6)


@pytest.mark.parametrize("visc", [(1.0, 0.0, 0.0, 3, 0), (1.0, 0.0, 1e-6, 0, 0), (1.0, 0.0, 1e-6, 2, 0)], ids=["fixed", "tol", "tol-min2"])
@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
def test_uniform_translation_is_left_alone(hip_lib, double, visc):
    p, pos, vel, _, _ = _scene("block", double)
    p = p.copy()
    p["viscosity"] = 0.0
    vel[:, :3] = np.array([0.3, -1.25, 2.0], vel.dtype)
    sc = (p, pos, vel, None, None)
    s = capi.Solver(p, len(pos), solver=capi.DFSPH, double=double, surface_tension=False)
    s.dfsph_configure(0.0, 2, 0.0, 0, 0)   # (no divergence solve: the velocities stay uniform)
    s.set_particles(pos, vel)
    s.step_partial(capi.STAGE_P_ADVECT)
    b = s.get("velAdv")
    s.close()
    assert np.ptp(b[:, :3], axis=0).max() == 0.0   # gravity alone
    s = capi.Solver(p, len(pos), solver=capi.DFSPH, double=double, surface_tension=False)
    s.dfsph_configure(0.0, 2, 0.0, 0, 0)
    s.set_particles(pos, vel)
    s.dfsph_set_viscosity(*visc)
    s.step_partial(capi.STAGE_P_ADVECT)
    info = s.dfsph_viscosity_info()
    assert info["iterations"] == 0 and info["residual"] == 0.0 and info["rhs_norm"] > 0
    assert s.get("velAdv").tobytes() == b.tobytes()
    s.close()


def _state(s):
    return [a.tobytes() for a in s.download(pressure=True)]


def test_off_is_a_context_that_was_never_configured(hip_lib):
    sc = _scene("dam")
    never = _ctx(sc)
    zero = _ctx(sc, visc=(0.0, 1.0, 1e-3, 1, 0))
    toggled = _ctx(sc, visc=(1.0, 1.0, 1e-3, 1, 0))
    toggled.dfsph_set_viscosity(0.0)
    for k in range(6):
        for s in (never, zero, toggled):
            s.step(1)
        assert _state(zero) == _state(never) and _state(toggled) == _state(never), k
    for s in (zero, toggled):
        with pytest.raises(capi.NereusError):
            s.dfsph_viscosity_info()
        s.close()
    never.close()


# ---- 5. in the step -----------------------------------------------------------------------------------------------------------------------------------
def test_ten_steps_with_akinci_and_an_emitter(hip_lib):
    p, pos, vel, bi, vbi = _scene("dam")
    vel = vel * 0   # the dam break at rest
    s = _ctx((p, pos, vel, bi, vbi), visc=(1.0, 0.5, 1e-3, 1, 0), capacity=len(pos) + 600, dfsph=(0.0, 3, 0.0, 1, 1))
    s.surface_akinci(0.05, 0.02)
    # a disc above the column, pouring down: a layer of sites every fourth step
    s.emitter_set(0, center=(0.25, 0.6, 0.2), direction=(0.0, -1.0, 0.0), half_extent=2.5 / 32, speed=8.0, spacing=1.0 / 32, shape=capi.EMITTER_DISC)
    counts = []
    for k in range(10):
        s.step(1)
        info = s.dfsph_viscosity_info()
        counts.append(s.n)
        assert s.last_iterations == 3                      # nrs_last_iterations still reports the density solve
        assert info["on"] and 1 <= info["iterations"] <= 100 and info["residual"] <= 1e-3 * info["rhs_norm"], (k, info)
    assert counts[-1] > len(pos) and len(set(counts)) > 1    # the emitter changed the particle count mid-run
    gp, gv = s.download()
    assert np.isfinite(gp).all() and np.isfinite(gv).all()
    # P_ADVECT of the next step leaves the viscous velocity in NRS_ARR_VEL_ADV, the stage's time holds the solve
    s.set_profiling([capi.STAGE_P_ADVECT])
    s.step_partial(capi.STAGE_P_ADVECT)
    assert np.isfinite(s.get("velAdv")).all()
    s.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def _code(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except capi.NereusError as e:
        return int(re.search(r"error (-?\d+)", str(e)).group(1))
    return 0


def test_refusals(hip_lib):
    p, pos, vel, bi, vbi = _scene("dam")
    for solver in (capi.SESPH, capi.IISPH, capi.PCISPH, capi.PBF):
        s = capi.Solver(p, len(pos), solver=solver)
        assert _code(s.dfsph_set_viscosity, 1.0) == E_STATE
        assert _code(s.dfsph_set_viscosity, 0.0) == E_STATE
        assert _code(s.dfsph_viscosity_info) == E_STATE
        s.close()
    s = _ctx((p, pos, vel, bi, vbi))
    assert _code(s.dfsph_viscosity_info) == E_STATE                       # off
    for args in ((-1.0,), (float("nan"),), (float("inf"),), (1.0, -1.0), (1.0, float("nan")), (1.0, 0.0, 1.0), (1.0, 0.0, -1e-9),
                 (1.0, 0.0, float("nan")), (1.0, 0.0, 0.0, 0, 0), (1.0, 0.0, 1e-3, 5, 4)):
        assert _code(s.dfsph_set_viscosity, *args) == E_INVALID, args
    assert _code(s.dfsph_set_viscosity, 1.0, 0.0, 0.0, 1, 0) == 0
    assert _code(s.dfsph_set_viscosity, 1.0, 0.0, 0.999, 0, 0) == 0
    assert _code(s.dfsph_set_viscosity, 1.0, 1.0, 1e-3, 3, 3) == 0
    assert _code(s.dfsph_viscosity_info) == E_STATE                       # on, before a step
    s.step(1)
    assert s.dfsph_viscosity_info()["on"]
    # wall friction and moving bodies exclude each other, in both orders of the two calls
    body_of = np.zeros(len(bi), np.uint32)
    body_of[: len(bi) // 2] = 1
    assert _code(s.set_boundary_bodies, body_of, 2) == E_STATE
    assert _code(s.dfsph_set_viscosity, 1.0, 0.0, 1e-3, 1, 0) == 0        # slip walls may move
    assert _code(s.set_boundary_bodies, body_of, 2) == 0
    assert _code(s.dfsph_set_viscosity, 1.0, 0.5, 1e-3, 1, 0) == E_STATE
    assert _code(s.dfsph_set_viscosity, 2.0, 0.0, 1e-3, 1, 0) == 0
    s.step(1)
    assert s.dfsph_viscosity_info()["iterations"] >= 1
    s.set_boundary_bodies(None, 0)
    assert _code(s.dfsph_set_viscosity, 1.0, 0.5, 1e-3, 1, 0) == 0
    s.close()
