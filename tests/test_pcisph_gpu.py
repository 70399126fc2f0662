"""PCISPH on the device (NRS_SOLVER_PCISPH): the advection stage against IISPH's, list-driven against reference-order kernels bit
for bit, the device against the float64 model (tests/pcisph_model.py), the exit rule, determinism, a stability run, the refusals of
the ABI, the host class and one step at config C3."""
import os
import subprocess

import numpy as np
import pytest

from nereus_amd import capi, scene
from tests import pcisph_model
from tests.common import compressed_block, rel_err, small_dam_break
from tests.oracle_lib import IISPH, SESPH, Oracle

pytestmark = pytest.mark.gpu


def _solver(p, pos, vel, bi=None, vbi=None, solver=capi.PCISPH, **kw):
    s = capi.Solver(p, len(pos), solver=solver, **kw)
    s.set_particles(pos, vel)
    s.set_boundaries(bi, vbi, update_grid=True)
    return s


def _scenes(double=False, kernel_set=1, squeeze=1.0):
    """compressed_block, and the small dam break with boundaries.  squeeze < 1 moves the dam-break column towards its lower corner
    by that factor (the lattice of the column is below rest density: at 0.87 the particles along the floor and the walls get
    positive pressures) and eases the block to spacing 0.76 h (the loop is not stable on the default 0.72 h block, DESIGN.md
    "PCISPH", and the model comparison should not measure its divergence)."""
    p, pos, vel = compressed_block(double=double, kernel_set=kernel_set, ratio=0.72 if squeeze == 1.0 else 0.76)
    p2, sc = small_dam_break(double=double, kernel_set=kernel_set)
    dpos = sc["pos"].copy()
    lo = dpos[:, :3].min(axis=0)
    dpos[:, :3] = (lo + (dpos[:, :3] - lo) * squeeze).astype(dpos.dtype)
    return [("block", p, pos, vel, None, None), ("dam", p2, dpos, sc["vel"], sc["bi"], sc["vbi"])]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kernel_set", [capi.MULLER, capi.MONAGHAN])
def test_advect_equals_iisph_displacement_forces(hip_lib, double, kernel_set):
    for name, p, pos, vel, bi, vbi in _scenes(double, kernel_set):
        vel = vel.copy()
        vel[:, 0] = 0.3 * np.sin(np.arange(len(pos)))   # moving particles: the viscosity terms are not zero
        got = []
        for solver, stage in ((capi.PCISPH, capi.STAGE_P_ADVECT), (capi.IISPH, capi.STAGE_I_DISPLACEMENT)):
            s = _solver(p, pos, vel, bi, vbi, solver=solver, double=double, kernel_set=kernel_set)
            s.step_partial(stage)
            got.append([s.get("velAdv"), s.get("forcesAdv"), s.get("dens")])
            s.close()
        for nm, a, b in zip(("velAdv", "forcesAdv", "dens"), *got):
            np.testing.assert_array_equal(a, b, err_msg="%s %s" % (name, nm))


def _bitwise_scenes():
    scenes = []
    p, pos, vel = compressed_block()
    scenes.append((p, pos, vel, None, None, False))
    p2, sc = small_dam_break(solver=IISPH)
    scenes.append((p2, sc["pos"], sc["vel"], sc["bi"], sc["vbi"], False))
    rng = np.random.default_rng(5)
    h = float(p["interactionRadius"][0])
    blob = np.ones((120, 4), np.float32)
    blob[:, :3] = (np.array([0.2, 0.1, -0.3]) + rng.uniform(-0.45 * h, 0.45 * h, (120, 3))).astype(np.float32)
    loose = np.ones((200, 4), np.float32)
    loose[:, :3] = (np.array([0.2, 0.1, -0.3]) + rng.uniform(-3 * h, 3 * h, (200, 3))).astype(np.float32)
    crowd = np.concatenate([blob, loose])
    scenes.append((p, crowd, np.zeros_like(crowd), None, None, True))
    tank = sc["tank"]
    h2 = float(p2["interactionRadius"][0])
    wblob = np.ones((120, 4), np.float32)
    wblob[:, :3] = (np.array([0.75 * tank[0], 0.6 * h2, 0.5 * tank[2]]) + rng.uniform(-0.45 * h2, 0.45 * h2, (120, 3))).astype(np.float32)
    walled = np.concatenate([sc["pos"], wblob])
    scenes.append((p2, walled, np.zeros_like(walled), sc["bi"], sc["vbi"], True))
    return scenes


def test_list_kernels_equal_reference_order_bitwise(hip_lib):
    """The four scenes of the IISPH list-versus-reference test: at P_ADVECT, at P_SOLVE and after three full steps."""
    adv = ["dens", "velAdv", "forcesAdv", "posPred"]
    solve = ["densCorr", "P_l", "forcesP", "posPred", "pres"]
    for k, (pp, pos, vel, bi, vbi, overflows) in enumerate(_bitwise_scenes()):
        if overflows:
            s = _solver(pp, pos, vel, bi, vbi)
            s.step(1)
            assert s.get_stat(capi.STAT_HIT_OVERFLOW) > 0   # the scene really takes the per-particle fallback
            s.close()
        outs = []
        for ref in (False, True):
            s = _solver(pp, pos, vel, bi, vbi, reference_order=ref)
            s.step_partial(capi.STAGE_P_ADVECT)
            got = [s.get(nm) for nm in adv]
            s.set_particles(pos, vel)
            s.step_partial(capi.STAGE_P_SOLVE)
            got += [s.get(nm) for nm in solve] + [np.array([s.last_iterations])]
            s.set_particles(pos, vel)
            s.step(3)
            got += list(s.download(pressure=True)) + [np.array([s.last_iterations])]
            outs.append(got)
            s.close()
        names = adv + solve + ["iters", "pos", "vel", "pressure", "iters3"]
        for nm, a, b in zip(names, *outs):
            np.testing.assert_array_equal(a, b, err_msg="scene %d %s" % (k, nm))


def _device_and_model(p, pos, vel, bi, vbi, double, ref, min_iters, cap, eta=0.01, kernel_set=capi.MULLER):
    s = _solver(p, pos, vel, bi, vbi, double=double, reference_order=ref, kernel_set=kernel_set)
    s.pcisph_configure(eta, min_iters)
    s.set_max_iterations(cap)
    s.step_partial(capi.STAGE_P_ADVECT)
    x, va = s.get("sortedPos"), s.get("velAdv")
    bs = s.get("bSorted") if bi is not None else None
    s.set_particles(pos, vel)
    s.step_partial(capi.STAGE_P_SOLVE)
    dev = {nm: s.get(nm) for nm in ("densCorr", "P_l", "forcesP", "posPred")}
    dev["iters"] = s.last_iterations
    dev["error"] = s.get_stat(capi.STAT_DENSITY_ERROR)
    dev["delta"] = s.get_stat(capi.STAT_PCISPH_DELTA)
    s.set_particles(pos, vel)
    s.step(1)
    dev["pos"], dev["vel"], dev["pressure"] = s.download(pressure=True)
    if kernel_set == capi.MONAGHAN:   # no list kernels for Monaghan (Features::listKernels): the context builds no hit lists
        with pytest.raises(capi.NereusError, match="error -4"):
            s.get_stat(capi.STAT_HIT_MEAN)
    s.close()
    m = pcisph_model.run(p, x, va, None if bs is None else bs[:, :3], None if bs is None else bs[:, 3], delta=dev["delta"],
                         min_iters=min_iters, cap=cap, eta=eta, kernel_set=kernel_set)
    return dev, m


@pytest.mark.parametrize("double,ref,tol", [(True, True, 1e-10), (False, False, 1e-4)])
def test_device_matches_model_fixed_iterations(hip_lib, double, ref, tol):
    for name, p, pos, vel, bi, vbi in _scenes(double, squeeze=0.87):
        dev, m = _device_and_model(p, pos, vel, bi, vbi, double, ref, 5, 5)
        assert dev["iters"] == m["iters"] == 5
        assert m["p"].max() > 0, name   # the solve has something to correct
        if bi is not None:
            # the boundary terms are exercised: particles next to the walls carry pressure, their boundary share of Fp is not zero,
            # and a wrong sign of that share would miss the bar by far
            near = m["near_boundary"]
            assert np.count_nonzero(m["p"][near] > 0) >= 50
            assert np.abs(m["fp_boundary"][near & (m["p"] > 0)]).max() > 0
            assert rel_err(m["fp"] - 2 * m["fp_boundary"], m["fp"]) > 100 * tol
        for nm, want in (("densCorr", m["rho"]), ("P_l", m["p"]), ("forcesP", m["fp"]), ("posPred", m["xs"])):
            got = dev[nm][:, :3] if want.ndim == 2 else dev[nm]
            assert rel_err(got, want) <= tol, (name, nm, rel_err(got, want))
        assert rel_err(dev["pos"][:, :3], m["pos"]) <= tol, name
        assert rel_err(dev["vel"][:, :3], m["vel"]) <= tol, name
        assert rel_err(dev["pressure"], m["p"]) <= tol, name
        assert abs(dev["error"] - m["errors"][-1]) <= 2 * tol, name


@pytest.mark.parametrize("double,ref", [(True, True), (False, False)])
def test_default_exit_rule_matches_model(hip_lib, double, ref):
    """Iteration counts agree wherever the model's max error is clear of eta (relative margin 1e-3), which is asserted first.  Cases:
    the 0.72 h block (runs to the cap), the dam break (no error from the start: stops at min_iters) and the dam-break column squeezed
    to 0.9 with min_iters = 1, whose loop converges and stops on max e <= eta after more than min_iters iterations."""
    cases = [(sc, 3) for sc in _scenes(double)]
    cases.append((_scenes(double, squeeze=0.9)[1], 1))
    for (name, p, pos, vel, bi, vbi), min_iters in cases:
        dev, m = _device_and_model(p, pos, vel, bi, vbi, double, ref, min_iters, 50)
        for l, e in enumerate(m["errors"], 1):
            if l >= min_iters:
                assert abs(e - 0.01) >= 1e-3 * 0.01, (name, l, e)
        assert dev["iters"] == m["iters"], (name, dev["iters"], m["iters"], m["errors"])
        if min_iters == 1:
            assert 1 < m["iters"] < 50 and m["errors"][-1] <= 0.01 < m["errors"][0], m["errors"]
            assert dev["error"] <= 0.01


def _monaghan_scenes(double, squeeze=0.7, ratio=0.68):
    """Monaghan densities at a given spacing are far below Muller's: the block at spacing 0.68 h (max rho* 1.2 rho0) and the dam-break
    column squeezed to 0.7 (its floor and wall particles compressed) give the solve something to correct.  The time step is 2e-4: with
    these parameters the Monaghan advection throws the particles next to the walls more than h off them in a step of 1e-3 (|vel_adv|
    ~ 66 m/s), after which no boundary term is left to test.  With the prototype's delta the Monaghan loop does not converge on either
    scene (its error grows over the iterations, DESIGN.md "PCISPH"), so the model comparison runs 3 fixed iterations."""
    p, pos, vel = compressed_block(double=double, kernel_set=capi.MONAGHAN, ratio=ratio)
    p2, sc = small_dam_break(double=double, kernel_set=capi.MONAGHAN)
    for q in (p, p2):
        q["timestep"] = 2e-4
    dpos = sc["pos"].copy()
    lo = dpos[:, :3].min(axis=0)
    dpos[:, :3] = (lo + (dpos[:, :3] - lo) * squeeze).astype(dpos.dtype)
    return [("block", p, pos, vel, None, None), ("dam", p2, dpos, sc["vel"], sc["bi"], sc["vbi"])]


@pytest.mark.parametrize("double,tol", [(True, 1e-10), (False, 1e-4)])
@pytest.mark.parametrize("ref", [False, True])
def test_monaghan_device_matches_model_fixed_iterations(hip_lib, double, tol, ref):
    """The Monaghan branch of W_dens / W_grad and of k_pci_prototype against the model's independent restatement (pinned to the
    reference's Wmonaghan / Wmonaghan_grad by tests/test_model_kernels_pin.py), with the bars of the Muller test."""
    for name, p, pos, vel, bi, vbi in _monaghan_scenes(double):
        dev, m = _device_and_model(p, pos, vel, bi, vbi, double, ref, 3, 3, kernel_set=capi.MONAGHAN)
        want, count = pcisph_model.prototype_delta(p, kernel_set=capi.MONAGHAN)
        assert count == 6
        np.testing.assert_allclose(dev["delta"], want, rtol=1e-5)
        assert abs(want / pcisph_model.prototype_delta(p)[0] - 1) > 1   # (not the Muller prototype's delta)
        assert dev["iters"] == m["iters"] == 3
        assert m["p"].max() > 0, name
        if bi is not None:
            near = m["near_boundary"]
            assert np.count_nonzero(m["p"][near] > 0) >= 50
            assert np.abs(m["fp_boundary"][near & (m["p"] > 0)]).max() > 0
            assert rel_err(m["fp"] - 2 * m["fp_boundary"], m["fp"]) > 100 * tol
        for nm, want in (("densCorr", m["rho"]), ("P_l", m["p"]), ("forcesP", m["fp"]), ("posPred", m["xs"])):
            got = dev[nm][:, :3] if want.ndim == 2 else dev[nm]
            assert rel_err(got, want) <= tol, (name, nm, rel_err(got, want))
        assert rel_err(dev["pos"][:, :3], m["pos"]) <= tol, name
        assert rel_err(dev["vel"][:, :3], m["vel"]) <= tol, name
        assert rel_err(dev["pressure"], m["p"]) <= tol, name
        assert abs(dev["error"] - m["errors"][-1]) <= 2 * tol, name


@pytest.mark.parametrize("double,ref", [(True, True), (False, False)])
def test_monaghan_exit_rule_matches_model(hip_lib, double, ref):
    """Monaghan, default exit rule: the 0.68 h block runs to the cap (every error after min_iters well above eta) and the dam break
    squeezed only to 0.8 has no error from the start (stops at min_iters)."""
    block = _monaghan_scenes(double)[0]
    dam = _monaghan_scenes(double, squeeze=0.8)[1]
    for (name, p, pos, vel, bi, vbi), want in ((block, 50), (dam, 3)):
        dev, m = _device_and_model(p, pos, vel, bi, vbi, double, ref, 3, 50, kernel_set=capi.MONAGHAN)
        for l, e in enumerate(m["errors"], 1):
            if l >= 3:
                assert abs(e - 0.01) >= 1e-3 * 0.01, (name, l, e)
        assert dev["iters"] == m["iters"] == want, (name, dev["iters"], m["iters"], m["errors"])
        if want == 50:
            assert min(m["errors"][2:]) > 0.05 and dev["error"] > 0.01


def test_delta_and_convergence_on_compressed_block(hip_lib):
    p, pos, vel = compressed_block()
    want, count = pcisph_model.prototype_delta(p)
    assert count == 6
    s = _solver(p, pos, vel)
    s.step(1)
    np.testing.assert_allclose(s.get_stat(capi.STAT_PCISPH_DELTA), want, rtol=1e-5)
    l = s.last_iterations
    err = s.get_stat(capi.STAT_DENSITY_ERROR)
    assert l >= 3
    assert err <= 0.01 or l == 50, (l, err)
    s.close()
    s = _solver(p, pos, vel)
    s.pcisph_configure(0.01, 1)
    s.set_max_iterations(1)
    s.step(1)
    assert s.last_iterations == 1
    first = s.get_stat(capi.STAT_DENSITY_ERROR)
    s.close()
    # A finding, not a property: on this block (spacing 0.72 h, 34 % over rest density) the loop as defined does not converge — the
    # error after 50 iterations is above the one after the first (DESIGN.md "PCISPH"; the model diverges the same way).  Pinned so
    # that a change of behaviour shows up here.
    assert first > 0.01 and l == 50 and err > first, (err, first, l)


def test_coherent_resort_and_batched_steps_are_deterministic(hip_lib):
    p, sc = small_dam_break((36, 34, 32))
    n = len(sc["pos"])
    assert n >= 32768
    names = ("hash", "index", "dens", "P_l", "forcesP", "posPred")
    outs = []
    for flags in (0, capi.FLAG_FULL_SORT):
        s = _solver(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"], flags=flags)
        s.step(3)
        s.step(4)
        outs.append(s.download(pressure=True) + tuple(s.get(x) for x in names) + (s.last_iterations,))
        if flags == 0:
            assert s.resort_stats() == (6, 0)
        s.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    p, pos, vel = compressed_block()
    outs = []
    for batched in (True, False):
        s = _solver(p, pos, vel)
        if batched:
            s.step(20)
        else:
            for _ in range(20):
                s.step(1)
        outs.append(s.download(pressure=True) + (s.last_iterations,))
        s.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


def test_small_dam_break_stays_in_the_tank(hip_lib):
    p, sc = small_dam_break()
    p = p.copy()
    p["timestep"] = 2.5e-4
    s = _solver(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
    h = float(p["interactionRadius"][0])
    tank = np.array(sc["tank"])
    lo, hi = sc["bi"][:, :3].min(axis=0) - h, sc["bi"][:, :3].max(axis=0) + h
    for _ in range(4):
        s.step(100)
        pos, vel = s.download()
        assert np.all(np.isfinite(pos)) and np.all(np.isfinite(vel))
        assert np.all(pos[:, :3] >= lo) and np.all(pos[:, :3] <= hi), (pos[:, :3].min(axis=0), pos[:, :3].max(axis=0), lo, hi)
        assert s.get_stat(capi.STAT_DENSITY_ERROR) <= 0.01 or s.last_iterations == 50
    assert tank[0] > 0
    s.close()


def test_abi_refusals(hip_lib):
    p, pos, vel = compressed_block()
    s = _solver(p, pos, vel)
    for args in ((0.0, 3, 0.0, 0.0), (-1.0, 3, 0.0, 0.0), (0.01, 0, 0.0, 0.0), (0.01, 3, -1.0, 0.0), (0.01, 3, 0.0, -1.0)):
        with pytest.raises(capi.NereusError, match="error -1"):
            s.pcisph_configure(*args)
    with pytest.raises(capi.NereusError, match="error -1"):
        s.slab_configure(0, 64, 8)
    for call in (s.iisph_predict, s.iisph_iterate, s.iisph_finish):
        with pytest.raises(capi.NereusError, match="error -4"):
            call()
    for stage in (capi.STAGE_FORCES, capi.STAGE_INTEGRATE, capi.STAGE_I_DENSITY, capi.STAGE_I_SOLVE, capi.STAGE_I_INTEGRATE):
        with pytest.raises(capi.NereusError, match="error -1"):
            s.step_partial(stage)
    with pytest.raises(capi.NereusError, match="error -4"):
        s.get_stat(capi.STAT_DENSITY_ERROR)       # no solve yet
    with pytest.raises(capi.NereusError, match="error -4"):
        s.get("aii")
    h = float(p["interactionRadius"][0])
    s.pcisph_configure(0.01, 3, 1.5 * h, 0.0)     # a prototype without neighbours: the step says so
    with pytest.raises(capi.NereusError, match="no neighbour"):
        s.step(1)
    s.pcisph_configure(0.01, 3, 0.0, 0.0)
    s.set_particles(pos, vel)
    s.step(1)
    assert 3 <= s.last_iterations <= 50
    s.close()
    for solver in (capi.SESPH, capi.IISPH):
        o = _solver(p, pos, vel, solver=solver)
        with pytest.raises(capi.NereusError, match="error -4"):
            o.pcisph_configure()
        with pytest.raises(capi.NereusError, match="error -4"):
            o.get("posPred")
        o.close()
    assert hip_lib.nrs_version() == 3


def test_host_class_pressure_solve_equals_capi(tmp_path, hip_lib):
    from tests.test_host_class import _driver, _read_out, _write_in
    p, sc = small_dam_break()
    pos, vel, bi, vbi = sc["pos"], sc["vel"], sc["bi"], sc["vbi"]
    steps = 5
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write_in(fin, pos, vel, bi, vbi)
    subprocess.check_call([_driver(), "run", "pcisph-solve", fin, str(steps), fout], stdout=subprocess.DEVNULL)
    got = _read_out(fout)
    s = _solver(Oracle.default_params(SESPH), pos, vel, bi, vbi)
    for _ in range(steps):
        s.step(1)
    gp, gv, gpr = s.download(pressure=True)
    np.testing.assert_array_equal(got["pos"], gp)
    np.testing.assert_array_equal(got["vel"], gv)
    np.testing.assert_array_equal(got["pressure"], gpr)
    assert got["iters"] == s.last_iterations > 0
    s.close()


def test_c3_one_step(hip_lib):
    """BASELINE config C3 (160^3 = 4,096,000 particles, fp32) with the IISPH constructor's parameters, as the IISPH C3 test"""
    p = Oracle.default_params(IISPH)
    sc = scene.dam_break("C3", h=float(p["interactionRadius"][0]), kpoly=float(p["kpoly"][0]))
    assert len(sc["pos"]) == 4_096_000
    s = _solver(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
    s.step(1)
    pos, vel = s.download()
    assert np.all(np.isfinite(pos)) and np.all(np.isfinite(vel))
    err = s.get_stat(capi.STAT_DENSITY_ERROR)
    assert err <= 0.01 or s.last_iterations == 50, (err, s.last_iterations)
    s.close()
