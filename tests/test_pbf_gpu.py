"""PBF on the device (NRS_SOLVER_PBF): the advection stage against PCISPH's, list-driven against reference-order kernels bit for bit,
the device against the float64 model (tests/pbf_model.py), the exit rules, determinism, a stability run, the refusals of the ABI, the
host class and one step at config C3."""
import subprocess

import numpy as np
import pytest

from nereus_amd import capi, scene
from tests import pbf_model
from tests.common import compressed_block, rel_err, small_dam_break
from tests.oracle_lib import IISPH, SESPH, Oracle
from tests.test_pcisph_gpu import _bitwise_scenes, _monaghan_scenes, _scenes, _solver

pytestmark = pytest.mark.gpu


def _pbf(p, pos, vel, bi=None, vbi=None, **kw):
    return _solver(p, pos, vel, bi, vbi, solver=capi.PBF, **kw)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kernel_set", [capi.MULLER, capi.MONAGHAN])
def test_advect_equals_pcisph(hip_lib, double, kernel_set):
    for name, p, pos, vel, bi, vbi in _scenes(double, kernel_set):
        vel = vel.copy()
        vel[:, 0] = 0.3 * np.sin(np.arange(len(pos)))
        got = []
        for solver in (capi.PBF, capi.PCISPH):
            s = _solver(p, pos, vel, bi, vbi, solver=solver, double=double, kernel_set=kernel_set)
            s.step_partial(capi.STAGE_P_ADVECT)
            got.append([s.get(nm) for nm in ("dens", "velAdv", "forcesAdv", "posPred")])
            s.close()
        for nm, a, b in zip(("dens", "velAdv", "forcesAdv", "posPred"), *got):
            np.testing.assert_array_equal(a, b, err_msg="%s %s" % (name, nm))


@pytest.mark.parametrize("xsph", [0.0, 0.1])
def test_list_kernels_equal_reference_order_bitwise(hip_lib, xsph):
    """The four scenes of the PCISPH test (compressed block, dam break with walls, and two crowded blobs that overflow their hit
    lists, one on the tank floor): at P_SOLVE (fixed 3 iterations, and the eta rule) and after three full steps."""
    solve = ["densCorr", "P_l", "forcesP", "posPred", "pres"]
    for k, (pp, pos, vel, bi, vbi, overflows) in enumerate(_bitwise_scenes()):
        if overflows:
            s = _pbf(pp, pos, vel, bi, vbi)
            s.step(1)
            assert s.get_stat(capi.STAT_HIT_OVERFLOW) > 0   # the scene really takes the per-particle fallback
            s.close()
        outs = []
        for ref in (False, True):
            s = _pbf(pp, pos, vel, bi, vbi, reference_order=ref)
            got = []
            for eta in (0.0, 0.01):
                s.pbf_configure(eta, 3, 0.01, xsph)
                s.set_particles(pos, vel)
                s.step_partial(capi.STAGE_P_SOLVE)
                got += [s.get(nm) for nm in solve] + [np.array([s.last_iterations, s.get_stat(capi.STAT_DENSITY_ERROR)])]
            s.set_particles(pos, vel)
            s.step(3)
            got += list(s.download(pressure=True)) + [np.array([s.last_iterations])]
            outs.append(got)
            s.close()
        names = ["fixed " + x for x in solve + ["iters"]] + ["eta " + x for x in solve + ["iters"]] + ["pos", "vel", "pressure", "iters3"]
        for nm, a, b in zip(names, *outs):
            np.testing.assert_array_equal(a, b, err_msg="scene %d %s" % (k, nm))


def _device_and_model(p, pos, vel, bi, vbi, double, ref, min_iters, cap=50, eta=0.0, xsph=0.0, kernel_set=capi.MULLER):
    s = _pbf(p, pos, vel, bi, vbi, double=double, reference_order=ref, kernel_set=kernel_set)
    s.pbf_configure(eta, min_iters, 0.01, xsph)
    s.set_max_iterations(cap)
    s.step_partial(capi.STAGE_P_ADVECT)
    x, va = s.get("sortedPos"), s.get("velAdv")
    bs = s.get("bSorted") if bi is not None else None
    s.set_particles(pos, vel)
    s.step_partial(capi.STAGE_P_SOLVE)
    dev = {nm: s.get(nm) for nm in ("densCorr", "P_l", "forcesP", "posPred")}
    dev["iters"] = s.last_iterations
    dev["error"] = s.get_stat(capi.STAT_DENSITY_ERROR)
    dev["eps"] = s.get_stat(capi.STAT_PBF_EPSILON)
    s.set_particles(pos, vel)
    s.step(1)
    dev["pos"], dev["vel"], dev["pressure"] = s.download(pressure=True)
    if kernel_set == capi.MONAGHAN:   # no list kernels for Monaghan (Features::listKernels): the context builds no hit lists
        with pytest.raises(capi.NereusError, match="error -4"):
            s.get_stat(capi.STAT_HIT_MEAN)
    s.close()
    m = pbf_model.run(p, x, va, None if bs is None else bs[:, :3], None if bs is None else bs[:, 3], eps=dev["eps"],
                      min_iters=min_iters, cap=cap, eta=eta, xsph=xsph, kernel_set=kernel_set)
    return dev, m


@pytest.mark.parametrize("double,tol", [(False, 1e-4), (True, 1e-10)])
@pytest.mark.parametrize("ref", [False, True])
@pytest.mark.parametrize("iters", [1, 3])
def test_device_matches_model_fixed_iterations(hip_lib, double, tol, ref, iters):
    for name, p, pos, vel, bi, vbi in _scenes(double, squeeze=0.87):
        xsph = 0.1 if iters == 3 else 0.0
        dev, m = _device_and_model(p, pos, vel, bi, vbi, double, ref, iters, cap=1, xsph=xsph)
        assert dev["iters"] == m["iters"] == iters   # (fixed-count mode: the cap of 1 does not apply)
        np.testing.assert_allclose(dev["eps"], 0.01 * pbf_model.prototype_d(p)[0], rtol=1e-5)
        assert m["lam"].min() < 0, name   # the solve has something to correct
        if bi is not None:   # the boundary terms are exercised: particles with a wall particle within h are compressed
            near = pbf_model._len(m["xs"][:, None, :] - bi[None, :, :3]).min(axis=1) < float(p["interactionRadius"][0])
            assert np.count_nonzero(m["lam"][near] < 0) >= 50, name
        for nm, want in (("densCorr", m["rho"]), ("P_l", m["lam"]), ("forcesP", m["dx"]), ("posPred", m["xs"])):
            got = dev[nm][:, :3] if want.ndim == 2 else dev[nm]
            assert rel_err(got, want) <= tol, (name, nm, rel_err(got, want))
        assert rel_err(dev["pos"][:, :3], m["pos"]) <= tol, name
        assert rel_err(dev["vel"][:, :3], m["vel"]) <= 10 * tol, (name, rel_err(dev["vel"][:, :3], m["vel"]))
        assert rel_err(dev["pressure"], m["lam"]) <= tol, name
        assert abs(dev["error"] - m["errors"][-1]) <= 2 * tol, name


@pytest.mark.parametrize("double,ref", [(True, True), (False, False)])
def test_exit_rule_matches_model(hip_lib, double, ref):
    """Iteration counts agree wherever the model's max error is clear of eta (relative margin 1e-3), which is asserted first: the
    compressed block with min_iters 1 (converges after more than min_iters iterations) and the dam break squeezed to 0.87."""
    for name, p, pos, vel, bi, vbi in _scenes(double, squeeze=0.87):
        if name == "block":
            p, pos, vel = compressed_block(double=double)
        dev, m = _device_and_model(p, pos, vel, bi, vbi, double, ref, 1, eta=0.01)
        for e in m["errors"]:
            assert abs(e - 0.01) >= 1e-3 * 0.01, (name, m["errors"])
        assert dev["iters"] == m["iters"], (name, dev["iters"], m["iters"], m["errors"])
        assert dev["error"] <= 0.01 or dev["iters"] == 50
        if name == "block":
            assert 1 < m["iters"] < 50 and m["errors"][-1] <= 0.01 < m["errors"][0], m["errors"]


@pytest.mark.parametrize("double,tol", [(False, 1e-4), (True, 1e-10)])
@pytest.mark.parametrize("ref", [False, True])
@pytest.mark.parametrize("iters", [1, 3])
def test_monaghan_device_matches_model_fixed_iterations(hip_lib, double, tol, ref, iters):
    """The Monaghan branch of W_dens / pbf_grad and of k_pbf_prototype against the model (tests/test_pcisph_gpu.py's Monaghan scenes:
    the 0.68 h block and the dam break squeezed to 0.7, time step 2e-4), with the bars of the Muller test.  The Monaghan loop relaxes
    the layer along the walls faster: after 3 iterations at least 25 particles next to a wall are still compressed (Muller: 50)."""
    for name, p, pos, vel, bi, vbi in _monaghan_scenes(double):
        xsph = 0.1 if iters == 3 else 0.0
        dev, m = _device_and_model(p, pos, vel, bi, vbi, double, ref, iters, cap=1, xsph=xsph, kernel_set=capi.MONAGHAN)
        assert dev["iters"] == m["iters"] == iters
        want = 0.01 * pbf_model.prototype_d(p, capi.MONAGHAN)[0]
        np.testing.assert_allclose(dev["eps"], want, rtol=1e-5)
        assert abs(want / (0.01 * pbf_model.prototype_d(p)[0]) - 1) > 0.5   # (not the Muller prototype's eps)
        assert m["lam"].min() < 0, name
        if bi is not None:
            near = pbf_model._len(m["xs"][:, None, :] - bi[None, :, :3]).min(axis=1) < float(p["interactionRadius"][0])
            assert np.count_nonzero(m["lam"][near] < 0) >= (50 if iters == 1 else 25), name
        for nm, want in (("densCorr", m["rho"]), ("P_l", m["lam"]), ("forcesP", m["dx"]), ("posPred", m["xs"])):
            got = dev[nm][:, :3] if want.ndim == 2 else dev[nm]
            assert rel_err(got, want) <= tol, (name, nm, rel_err(got, want))
        assert rel_err(dev["pos"][:, :3], m["pos"]) <= tol, name
        assert rel_err(dev["vel"][:, :3], m["vel"]) <= 10 * tol, (name, rel_err(dev["vel"][:, :3], m["vel"]))
        assert rel_err(dev["pressure"], m["lam"]) <= tol, name
        assert abs(dev["error"] - m["errors"][-1]) <= 2 * tol, name


@pytest.mark.parametrize("double,ref", [(True, True), (False, False)])
def test_monaghan_exit_rule_matches_model(hip_lib, double, ref):
    """Monaghan, eta rule with min_iters 1: the 0.68 h block converges after more than min_iters iterations, every error clear of
    eta (relative margin 1e-3)."""
    name, p, pos, vel, bi, vbi = _monaghan_scenes(double)[0]
    dev, m = _device_and_model(p, pos, vel, bi, vbi, double, ref, 1, eta=0.01, kernel_set=capi.MONAGHAN)
    for e in m["errors"]:
        assert abs(e - 0.01) >= 1e-3 * 0.01, m["errors"]
    assert dev["iters"] == m["iters"], (dev["iters"], m["iters"], m["errors"])
    assert 1 < m["iters"] < 50 and m["errors"][-1] <= 0.01 < m["errors"][0], m["errors"]
    assert dev["error"] <= 0.01


def test_fixed_count_mode_runs_exactly_min_iters(hip_lib):
    p, pos, vel = compressed_block()
    for min_iters, cap in ((1, 0), (4, 0), (7, 2)):
        s = _pbf(p, pos, vel)
        s.pbf_configure(0.0, min_iters)
        s.set_max_iterations(cap)
        s.step(2)
        assert s.last_iterations == min_iters
        assert s.get_stat(capi.STAT_DENSITY_ERROR) >= 0   # formed on request
        s.close()


def test_reaches_eta_on_compressed_block(hip_lib):
    p, pos, vel = compressed_block()
    s = _pbf(p, pos, vel)
    s.pbf_configure(0.01, 2)
    s.step(1)
    l, err = s.last_iterations, s.get_stat(capi.STAT_DENSITY_ERROR)
    assert 2 <= l < 50 and err <= 0.01, (l, err)
    np.testing.assert_allclose(s.get_stat(capi.STAT_PBF_EPSILON), 0.01 * pbf_model.prototype_d(p)[0], rtol=1e-5)
    s.close()


def test_coherent_resort_and_batched_steps_are_deterministic(hip_lib):
    p, sc = small_dam_break((36, 34, 32))
    assert len(sc["pos"]) >= 32768
    names = ("hash", "index", "dens", "P_l", "forcesP", "posPred")
    for eta, xsph in ((0.01, 0.0), (0.0, 0.1)):
        outs = []
        for flags, batched in ((0, True), (0, False), (capi.FLAG_FULL_SORT, True)):
            s = _pbf(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"], flags=flags)
            s.pbf_configure(eta, 3, 0.01, xsph)
            if batched:
                s.step(3)
                s.step(4)
            else:
                for _ in range(7):
                    s.step(1)
            outs.append(s.download(pressure=True) + tuple(s.get(x) for x in names) + (s.last_iterations,))
            if flags == 0:
                assert s.resort_stats() == (6, 0)
            s.close()
        for o in outs[1:]:
            for a, b in zip(outs[0], o):
                np.testing.assert_array_equal(a, b)


def test_small_dam_break_stays_in_the_tank(hip_lib):
    p, sc = small_dam_break()
    s = _pbf(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
    h = float(p["interactionRadius"][0])
    lo, hi = sc["bi"][:, :3].min(axis=0) - h, sc["bi"][:, :3].max(axis=0) + h
    for _ in range(4):
        s.step(50)
        pos, vel = s.download()
        assert np.all(np.isfinite(pos)) and np.all(np.isfinite(vel))
        assert np.all(pos[:, :3] >= lo) and np.all(pos[:, :3] <= hi), (pos[:, :3].min(axis=0), pos[:, :3].max(axis=0), lo, hi)
        assert s.get_stat(capi.STAT_DENSITY_ERROR) <= 0.01 or s.last_iterations == 50
    s.close()


def test_abi_refusals(hip_lib):
    p, pos, vel = compressed_block()
    s = _pbf(p, pos, vel)
    for args in ((-1.0, 2, 0.01, 0.0), (0.01, 0, 0.01, 0.0), (0.01, 2, 0.0, 0.0), (0.01, 2, -1.0, 0.0), (0.01, 2, 0.01, -0.1),
                 (0.01, 2, 0.01, 1.5), (float("nan"), 2, 0.01, 0.0)):
        with pytest.raises(capi.NereusError, match="error -1"):
            s.pbf_configure(*args)
    with pytest.raises(capi.NereusError, match="error -4"):
        s.pcisph_configure()
    with pytest.raises(capi.NereusError, match="error -1"):
        s.slab_configure(0, 64, 8)
    for call in (s.iisph_predict, s.iisph_iterate, s.iisph_finish):
        with pytest.raises(capi.NereusError, match="error -4"):
            call()
    for stage in (capi.STAGE_FORCES, capi.STAGE_INTEGRATE, capi.STAGE_I_DENSITY, capi.STAGE_I_SOLVE, capi.STAGE_I_INTEGRATE):
        with pytest.raises(capi.NereusError, match="error -1"):
            s.step_partial(stage)
    for stat in (capi.STAT_DENSITY_ERROR, capi.STAT_PBF_EPSILON):
        with pytest.raises(capi.NereusError, match="error -4"):
            s.get_stat(stat)   # no solve yet
    with pytest.raises(capi.NereusError, match="error -4"):
        s.get_stat(capi.STAT_PCISPH_DELTA)
    with pytest.raises(capi.NereusError, match="error -4"):
        s.get("aii")
    s.pbf_configure(0.01, 2, 0.01, 1.0)   # the ends of the ranges are accepted
    s.pbf_configure(0.0, 1, 1e-6, 0.0)
    s.pbf_configure()
    s.set_particles(pos, vel)
    s.step(1)
    assert 2 <= s.last_iterations <= 50
    s.close()
    for solver in (capi.SESPH, capi.IISPH, capi.PCISPH):
        o = _solver(p, pos, vel, solver=solver)
        with pytest.raises(capi.NereusError, match="error -4"):
            o.pbf_configure()
        if solver != capi.PCISPH:
            with pytest.raises(capi.NereusError, match="error -4"):
                o.get("posPred")
        o.step(1)
        with pytest.raises(capi.NereusError, match="error -4"):
            o.get_stat(capi.STAT_PBF_EPSILON)
        o.close()
    assert hip_lib.nrs_version() == 3


def test_host_class_equals_capi(tmp_path, hip_lib):
    from tests.test_host_class import _driver, _read_out, _write_in
    p, sc = small_dam_break()
    pos, vel, bi, vbi = sc["pos"], sc["vel"], sc["bi"], sc["vbi"]
    steps = 5
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write_in(fin, pos, vel, bi, vbi)
    subprocess.check_call([_driver(), "run", "pbf", fin, str(steps), fout], stdout=subprocess.DEVNULL)
    got = _read_out(fout)
    s = _pbf(Oracle.default_params(SESPH), pos, vel, bi, vbi)
    for _ in range(steps):
        s.step(1)
    gp, gv, gpr = s.download(pressure=True)
    np.testing.assert_array_equal(got["pos"], gp)
    np.testing.assert_array_equal(got["vel"], gv)
    np.testing.assert_array_equal(got["pressure"], gpr)
    assert got["iters"] == s.last_iterations > 0
    s.close()


def test_c3_one_step(hip_lib):
    """BASELINE config C3 (160^3 = 4,096,000 particles, fp32) with the IISPH constructor's parameters"""
    p = Oracle.default_params(IISPH)
    sc = scene.dam_break("C3", h=float(p["interactionRadius"][0]), kpoly=float(p["kpoly"][0]))
    assert len(sc["pos"]) == 4_096_000
    s = _pbf(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
    s.step(1)
    pos, vel = s.download()
    assert np.all(np.isfinite(pos)) and np.all(np.isfinite(vel))
    err = s.get_stat(capi.STAT_DENSITY_ERROR)
    assert err <= 0.01 or s.last_iterations == 50, (err, s.last_iterations)
    s.close()
