"""DFSPH on the device (NRS_SOLVER_DFSPH): the advection stage against PCISPH's, list-driven against reference-order kernels bit for
bit, the device against the float64 model (tests/dfsph_model.py), the exit rules, the warm start, edge sizes, determinism across the
sort paths, a stability run, the refusals of the ABI, the host class and one step at config C3."""
import subprocess

import numpy as np
import pytest

from nereus_amd import capi, scene
from tests import dfsph_model
from tests.common import compressed_block, rel_err, small_dam_break
from tests.oracle_lib import IISPH, SESPH, Oracle
from tests.test_pcisph_gpu import _bitwise_scenes, _monaghan_scenes, _scenes, _solver

pytestmark = pytest.mark.gpu

FIXED = (0.0, 3, 0.0, 3, 1)   # nrs_dfsph_configure: 3 + 3 iterations, warm start on, nothing read back
ETA = (1e-3, 1, 1e-3, 1, 1)


def _dfsph(p, pos, vel, bi=None, vbi=None, **kw):
    return _solver(p, pos, vel, bi, vbi, solver=capi.DFSPH, **kw)


def _moving(vel, scale=0.3):
    """velocities with a divergence for the divergence solve to remove"""
    vel = vel.copy()
    k = np.arange(len(vel))
    vel[:, 0] = scale * np.sin(k)
    vel[:, 1] = scale * np.cos(0.7 * k)
    return vel


def _ctx(sc, cfg, cap=0, pre=0, **kw):
    p, pos, vel, bi, vbi = sc
    s = _dfsph(p, pos, vel, bi, vbi, **kw)
    s.dfsph_configure(*cfg)
    s.set_max_iterations(cap)
    if pre:
        s.step(pre)
    return s


def _stages(sc, cfg, cap=0, pre=0, **kw):
    """the sorted inputs and the results of each DFSPH stage of step pre + 1 (a fresh context per stage: the runs are deterministic)"""
    o = {}
    s = _ctx(sc, cfg, cap, pre, **kw)
    s.step_partial(capi.STAGE_DENSITY)
    for k, nm in (("x", "sortedPos"), ("v0", "sortedVel"), ("rho", "dens"), ("alpha", "dfsphAlpha"), ("Kv_prev", "dfsphKappaV"),
                  ("K_prev", "pres")):
        o[k] = s.get(nm)
    o["bs"] = s.get("bSorted") if sc[3] is not None else None
    s.close()
    s = _ctx(sc, cfg, cap, pre, **kw)
    s.step_partial(capi.STAGE_P_ADVECT)
    for k, nm in (("v_df", "sortedVel"), ("Kv", "dfsphKappaV"), ("velAdv0", "velAdv"), ("forcesAdv", "forcesAdv"), ("K_prev2", "pres")):
        o[k] = s.get(nm)
    o["div_iters"] = s.get_stat(capi.STAT_DFSPH_DIVERGENCE_ITERATIONS)
    o["div_avg"] = s.get_stat(capi.STAT_DFSPH_DIVERGENCE_AVG) if cfg[3] else None
    s.close()
    s = _ctx(sc, cfg, cap, pre, **kw)
    s.step_partial(capi.STAGE_P_SOLVE)
    for k, nm in (("vstar", "velAdv"), ("K", "pres"), ("kappa", "P_l"), ("rho_adv", "densCorr")):
        o[k] = s.get(nm)
    o["iters"] = s.last_iterations
    o["avg"], o["max"] = s.get_stat(capi.STAT_DFSPH_DENSITY_AVG), s.get_stat(capi.STAT_DENSITY_ERROR)
    s.close()
    np.testing.assert_array_equal(o["K_prev"], o["K_prev2"])   # the divergence solve leaves K alone
    return o


def _model(p, o, cfg, cap=0, kernel_set=capi.MULLER):
    eta, mn, eta_v, mn_v, warm = cfg
    bs = o["bs"]
    pairs = dfsph_model.Pairs(p, o["x"], None if bs is None else bs[:, :3], None if bs is None else bs[:, 3], kernel_set)
    alpha, _ = dfsph_model.factor(p, pairs, kernel_set)
    cap = cap or 100
    div = dfsph_model.solve(p, pairs, alpha, o["v0"], o["Kv_prev"], min_iters=mn_v, eta=eta_v, cap=cap, warm=warm) if mn_v else None
    den = dfsph_model.solve(p, pairs, alpha, o["velAdv0"], o["K_prev"], rho=o["rho"], min_iters=mn, eta=eta, cap=cap, warm=warm)
    return alpha, div, den


def _compare(p, o, cfg, tol, what, cap=0, kernel_set=capi.MULLER):
    alpha, div, den = _model(p, o, cfg, cap, kernel_set)
    assert rel_err(o["alpha"], alpha) <= tol, (what, "alpha", rel_err(o["alpha"], alpha))
    assert rel_err(o["rho"], dfsph_model.density(p, o["x"], None if o["bs"] is None else o["bs"][:, :3],
                                                 None if o["bs"] is None else o["bs"][:, 3], kernel_set)) <= tol, what
    if div is not None:
        assert o["div_iters"] == div["iters"], (what, o["div_iters"], div["avgs"])
        assert rel_err(o["v_df"][:, :3], div["u"]) <= tol, (what, "v_df", rel_err(o["v_df"][:, :3], div["u"]))
        assert rel_err(o["v_df"][:, :3] - o["v0"][:, :3], div["u"] - o["v0"][:, :3]) <= 10 * tol, (what, "dv")
        assert rel_err(o["Kv"], div["K"]) <= tol, (what, "Kv", rel_err(o["Kv"], div["K"]))
        assert abs(o["div_avg"] - div["avgs"][-1]) <= tol * max(div["avgs"][0], 1e-30), (what, o["div_avg"], div["avgs"])
    else:
        assert o["div_iters"] == 0
        np.testing.assert_array_equal(o["v_df"], o["v0"])
    assert o["iters"] == den["iters"], (what, o["iters"], den["avgs"])
    for k, want in (("vstar", den["u"]), ("K", den["K"]), ("kappa", den["kappa"]), ("rho_adv", den["rho_adv"])):
        got = o[k][:, :3] if want.ndim == 2 else o[k]
        assert rel_err(got, want) <= tol, (what, k, rel_err(got, want))
    dv = o["vstar"][:, :3] - o["velAdv0"][:, :3]
    assert rel_err(dv, den["u"] - o["velAdv0"][:, :3]) <= 10 * tol, (what, "dv*", rel_err(dv, den["u"] - o["velAdv0"][:, :3]))
    assert abs(o["avg"] - den["avgs"][-1]) <= tol * den["avgs"][0], (what, o["avg"], den["avgs"])
    assert abs(o["max"] - den["maxes"][-1]) <= tol * den["maxes"][0], (what, o["max"], den["maxes"])
    return div, den


def _moving_scenes(double=False, kernel_set=capi.MULLER, squeeze=0.87):
    return [(name, (p, pos, _moving(vel), bi, vbi)) for name, p, pos, vel, bi, vbi in _scenes(double, kernel_set, squeeze)]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("kernel_set", [capi.MULLER, capi.MONAGHAN])
def test_advect_equals_pcisph_with_divergence_solve_off(hip_lib, double, kernel_set):
    for name, p, pos, vel, bi, vbi in _scenes(double, kernel_set):
        vel = _moving(vel)
        got = []
        for solver in (capi.DFSPH, capi.PCISPH):
            s = _solver(p, pos, vel, bi, vbi, solver=solver, double=double, kernel_set=kernel_set)
            if solver == capi.DFSPH:
                s.dfsph_configure(1e-3, 2, 1e-3, 0, 1)
            s.step_partial(capi.STAGE_P_ADVECT)
            got.append([s.get(nm) for nm in ("dens", "velAdv", "forcesAdv", "sortedVel")])
            s.close()
        for nm, a, b in zip(("dens", "velAdv", "forcesAdv", "sortedVel"), *got):
            np.testing.assert_array_equal(a, b, err_msg="%s %s" % (name, nm))


def test_list_kernels_equal_reference_order_bitwise(hip_lib):
    """The four scenes of the PCISPH test (compressed block, dam break with walls, and two crowded blobs that overflow their hit
    lists, one on the tank floor), moving: at DENSITY, P_ADVECT and P_SOLVE in fixed and eta modes, and after three full steps."""
    dens = ["dens", "dfsphAlpha", "pres", "dfsphKappaV"]
    adv = ["sortedVel", "velAdv", "forcesAdv", "dfsphKappaV"]
    solve = ["velAdv", "pres", "P_l", "densCorr"]
    for k, (pp, pos, vel, bi, vbi, overflows) in enumerate(_bitwise_scenes()):
        vel = _moving(vel)
        if overflows:
            s = _dfsph(pp, pos, vel, bi, vbi)
            s.step(1)
            assert s.get_stat(capi.STAT_HIT_OVERFLOW) > 0   # the scene really takes the per-particle fallback
            s.close()
        outs = []
        for ref in (False, True):
            s = _dfsph(pp, pos, vel, bi, vbi, reference_order=ref)
            got = []
            for cfg in (FIXED, ETA):
                s.dfsph_configure(*cfg)
                for stage, names in ((capi.STAGE_DENSITY, dens), (capi.STAGE_P_ADVECT, adv), (capi.STAGE_P_SOLVE, solve)):
                    s.set_particles(pos, vel)
                    s.step_partial(stage)
                    got += [s.get(nm) for nm in names]
                got.append(np.array([s.last_iterations, s.get_stat(capi.STAT_DFSPH_DIVERGENCE_ITERATIONS),
                                     s.get_stat(capi.STAT_DFSPH_DENSITY_AVG), s.get_stat(capi.STAT_DENSITY_ERROR),
                                     s.get_stat(capi.STAT_DFSPH_DIVERGENCE_AVG)]))
            s.set_particles(pos, vel)
            s.step(3)
            got += list(s.download(pressure=True)) + [s.get("dfsphKappaV"), s.get("dfsphAlpha"),
                                                      np.array([s.last_iterations, s.get_stat(capi.STAT_DFSPH_DIVERGENCE_ITERATIONS)])]
            outs.append(got)
            s.close()
        names = [m + " " + x for m in ("fixed", "eta") for x in dens + adv + solve + ["stats"]] + ["pos", "vel", "pressure", "Kv3", "alpha3",
                                                                                                  "iters3"]
        assert len(names) == len(outs[0])
        for nm, a, b in zip(names, *outs):
            np.testing.assert_array_equal(a, b, err_msg="scene %d %s" % (k, nm))


@pytest.mark.parametrize("double,tol", [(False, 1e-4), (True, 1e-10)])
@pytest.mark.parametrize("ref", [False, True])
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("pre", [0, 1])
def test_device_matches_model_fixed_iterations(hip_lib, double, tol, ref, iters, pre):
    """Both scenes moving (the block at 0.76 h, the dam break squeezed to 0.87 with its walls), 1 and 3 iterations per loop; pre = 1:
    the second step, whose warm-start inputs K_prev and Kv_prev are not zero"""
    cfg = (0.0, iters, 0.0, iters, 1)
    for name, sc in _moving_scenes(double):
        o = _stages(sc, cfg, cap=1, pre=pre, double=double, reference_order=ref)
        if pre:
            assert o["K_prev"].max() > 0 and o["Kv_prev"].max() > 0, name
        div, den = _compare(sc[0], o, cfg, tol, (name, pre))
        assert div["iters"] == den["iters"] == iters   # (fixed-count mode: the cap of 1 does not apply)
        assert den["first_e"].max() > 0 and div["first_e"].max() > 0, name   # both solves have something to correct
        if sc[3] is not None:   # the boundary terms are exercised: particles with a wall particle within h are compressed
            near = np.zeros(len(o["x"]), bool)
            near[dfsph_model.Pairs(sc[0], o["x"], o["bs"][:, :3], o["bs"][:, 3]).bi] = True
            assert np.count_nonzero(den["first_e"][near] > 0) >= 50, name


@pytest.mark.parametrize("double,tol", [(False, 1e-4), (True, 1e-10)])
@pytest.mark.parametrize("ref", [False, True])
@pytest.mark.parametrize("iters", [1, 3])
def test_monaghan_device_matches_model_fixed_iterations(hip_lib, double, tol, ref, iters):
    """The Monaghan branch of W_dens / pbf_grad and of the prototype against the model, on tests/test_pcisph_gpu.py's Monaghan scenes
    (time step 2e-4), moving, over two steps"""
    cfg = (0.0, iters, 0.0, iters, 1)
    for name, p, pos, vel, bi, vbi in _monaghan_scenes(double):
        sc = (p, pos, _moving(vel), bi, vbi)
        for pre in (0, 1):
            o = _stages(sc, cfg, pre=pre, double=double, reference_order=ref, kernel_set=capi.MONAGHAN)
            div, den = _compare(p, o, cfg, tol, (name, pre), kernel_set=capi.MONAGHAN)
            if pre == 0:   # (3 iterations relax the Monaghan block below rest density in one step)
                assert den["first_e"].max() > 0, name
    s = _dfsph(p, pos, vel, bi, vbi, double=double, kernel_set=capi.MONAGHAN)
    s.step(1)
    with pytest.raises(capi.NereusError, match="error -4"):   # no list kernels for Monaghan: the context builds no hit lists
        s.get_stat(capi.STAT_HIT_MEAN)
    s.close()


@pytest.mark.parametrize("double,ref", [(True, True), (False, False), (False, True)])
@pytest.mark.parametrize("pre", [0, 1])
def test_exit_rule_matches_model(hip_lib, double, ref, pre):
    """eta 1e-3 for both loops, min 1: the iteration counts of both loops equal the model's wherever every average is clear of eta
    (relative margin 1e-3, asserted first).  The compressed 0.72 h block needs several density iterations."""
    p, pos, vel = compressed_block(double=double)
    p2, sc2 = small_dam_break(double=double)
    for name, sc in (("block", (p, pos, _moving(vel), None, None)), ("dam", (p2, sc2["pos"], _moving(sc2["vel"]), sc2["bi"], sc2["vbi"]))):
        o = _stages(sc, ETA, pre=pre, double=double, reference_order=ref)
        _, div, den = _model(sc[0], o, ETA)
        for e in div["avgs"] + den["avgs"]:
            assert abs(e - 1e-3) >= 1e-3 * 1e-3, (name, div["avgs"], den["avgs"])
        assert o["div_iters"] == div["iters"] and o["iters"] == den["iters"], (name, o["div_iters"], div["avgs"], o["iters"], den["avgs"])
        assert o["avg"] <= 1e-3 or o["iters"] == 100
        if name == "block" and pre == 0:
            assert 1 < den["iters"] < 100 and den["avgs"][-1] <= 1e-3 < den["avgs"][0], den["avgs"]


def test_fixed_count_mode_and_the_cap(hip_lib):
    p, pos, vel = compressed_block()
    sc = (p, pos, _moving(vel), None, None)
    for mn, mn_v, cap in ((1, 1, 0), (4, 2, 0), (7, 5, 2)):
        s = _ctx(sc, (0.0, mn, 0.0, mn_v, 1), cap=cap)
        s.step(2)
        assert s.last_iterations == mn and s.get_stat(capi.STAT_DFSPH_DIVERGENCE_ITERATIONS) == mn_v
        assert s.get_stat(capi.STAT_DENSITY_ERROR) >= s.get_stat(capi.STAT_DFSPH_DENSITY_AVG) >= 0   # formed on request
        assert s.get_stat(capi.STAT_DFSPH_DIVERGENCE_AVG) >= 0
        s.close()
    s = _ctx(sc, (1e-12, 1, 1e-12, 1, 1), cap=3)   # an eta no loop reaches in 3 iterations: the cap ends both
    s.step(1)
    assert s.last_iterations == 3 and s.get_stat(capi.STAT_DFSPH_DIVERGENCE_ITERATIONS) == 3
    s.close()
    s = _ctx(sc, (1e-12, 1, 1e-12, 1, 1), cap=0)   # 0 = 100, not PBF's 50: the density loop needs more than 50 here
    s.step(1)
    assert 50 < s.last_iterations <= 100
    assert s.last_iterations == 100 or s.get_stat(capi.STAT_DFSPH_DENSITY_AVG) <= 1e-12
    s.close()


@pytest.mark.parametrize("ref", [False, True])
def test_warm_start_from_zero_is_bitwise_warm_start_off(hip_lib, ref):
    """After an upload K_prev = Kv_prev = 0: the warm pair changes nothing, in either mode of the loops"""
    p2, sc2 = small_dam_break()
    p, pos, vel = compressed_block()
    for sc in ((p, pos, _moving(vel), None, None), (p2, sc2["pos"], _moving(sc2["vel"]), sc2["bi"], sc2["vbi"])):
        for cfg in (FIXED, ETA):
            outs = []
            for warm in (1, 0):
                s = _ctx(sc, cfg[:4] + (warm,), reference_order=ref)
                s.step(1)
                outs.append(list(s.download(pressure=True)) + [s.get("dfsphKappaV"), s.get("P_l"), s.get("densCorr"),
                                                               np.array([s.last_iterations, s.get_stat(capi.STAT_DFSPH_DIVERGENCE_ITERATIONS)])])
                s.close()
            for a, b in zip(*outs):
                np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("ref", [False, True])
def test_translation_is_unchanged_and_momentum_holds(hip_lib, ref):
    """A uniformly translated block has no divergence: the divergence solve leaves the sorted velocities unchanged bit for bit.  With
    random velocities (fp64, no boundaries) both solves conserve momentum to roundoff."""
    p, pos, vel = compressed_block(ratio=0.76)
    vel = np.tile(np.array([0.31, -1.7, 0.05, 0.0], np.float32), (len(pos), 1))
    o = _stages((p, pos, vel, None, None), (1e-3, 2, 1e-3, 3, 1), reference_order=ref)
    np.testing.assert_array_equal(o["v_df"], o["v0"])
    assert o["div_avg"] == 0 and o["div_iters"] == 3
    p, pos, vel = compressed_block(double=True)
    rng = np.random.default_rng(11)
    vel = vel.copy()
    vel[:, :3] = rng.normal(0.0, 0.5, (len(pos), 3))
    o = _stages((p, pos, vel, None, None), (0.0, 3, 0.0, 3, 1), double=True, reference_order=ref)
    for a, b in ((o["v0"], o["v_df"]), (o["velAdv0"], o["vstar"])):
        assert np.abs(b - a).max() > 1e-4
        dp = (b[:, :3] - a[:, :3]).sum(axis=0)
        assert np.abs(dp).max() <= 1e-12 * np.abs(a[:, :3]).sum(), dp


def _edge_model(sc, ref, iters=2):
    cfg = (0.0, iters, 0.0, iters, 1)
    o = _stages(sc, cfg, pre=1, reference_order=ref)
    _compare(sc[0], o, cfg, 1e-4, len(sc[1]))
    return o


@pytest.mark.parametrize("ref", [False, True])
def test_edge_sizes_and_walls(hip_lib, ref):
    """0, 1, 63-65 and 255-257 particles of the 0.76 h block (moving), and the squeezed dam break with its walls, against the model
    over the second step"""
    p, pos, vel = compressed_block(ratio=0.76)
    vel = _moving(vel)
    s = capi.Solver(p, 16, solver=capi.DFSPH, reference_order=ref)
    s.step(2)   # empty: a no-op
    assert s.n == 0
    for arr in ("dfsphAlpha", "dfsphKappaV"):
        with pytest.raises(capi.NereusError, match="error -4"):
            s.get(arr)   # before a step
    s.close()
    one = np.array([[0.1, 0.2, 0.3, 1.0]], np.float32)
    o = _edge_model((p, one, np.array([[0.2, 0.0, 0.0, 0.0]], np.float32), None, None), ref)
    assert o["alpha"][0] == 0 and o["v_df"][0, 0] == np.float32(0.2)   # no neighbour: D = 0, nothing to correct
    for n in (63, 64, 65, 255, 256, 257):
        _edge_model((p, pos[:n], vel[:n], None, None), ref)
    (name, sc), = [x for x in _moving_scenes() if x[0] == "dam"]
    _edge_model(sc, ref)


@pytest.mark.parametrize("ref", [False, True])
def test_append_between_steps_equals_fresh_context(hip_lib, ref):
    """Two steps of the 0.76 h block, then 10 particles appended: the next step equals a fresh context loaded with the concatenated
    state and K as the pressure, bit for bit.  (The divergence solve is off: an upload restarts Kv at zero, DESIGN.md "DFSPH".)"""
    p, pos, vel = compressed_block(ratio=0.76)
    vel = _moving(vel)
    rng = np.random.default_rng(3)
    h = float(p["interactionRadius"][0])
    extra = np.ones((10, 4), np.float32)
    extra[:, :3] = (pos[:10, :3] + rng.uniform(-0.3 * h, 0.3 * h, (10, 3))).astype(np.float32)
    cfg = (0.0, 3, 0.0, 0, 1)
    s = capi.Solver(p, len(pos) + 64, solver=capi.DFSPH, reference_order=ref)
    s.dfsph_configure(*cfg)
    s.set_particles(pos, vel)
    s.step(2)
    xp, xv, xk = s.download(pressure=True)
    assert xk.max() > 0
    s.set_particles(extra, None, first=s.n)
    assert s.n == len(pos) + 10
    s.step(1)
    got = list(s.download(pressure=True)) + [s.last_iterations]
    s.close()
    f = capi.Solver(p, len(pos) + 10, solver=capi.DFSPH, reference_order=ref)
    f.dfsph_configure(*cfg)
    f.set_particles(np.concatenate([xp, extra]), np.concatenate([xv, np.zeros_like(extra)]), np.concatenate([xk, np.zeros(10, xk.dtype)]))
    f.step(1)
    want = list(f.download(pressure=True)) + [f.last_iterations]
    f.close()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def test_coherent_resort_and_batched_steps_are_deterministic(hip_lib):
    """The warm-start carry (K, Kv) survives both sort paths: the coherent re-sort against NRS_FLAG_FULL_SORT, and nrs_step(ctx, k)
    against k single steps, bit for bit"""
    p, sc = small_dam_break((36, 34, 32))
    assert len(sc["pos"]) >= 32768
    vel = _moving(sc["vel"], 0.1)
    pos = sc["pos"].copy()   # squeezed towards the floor: compressed, so K is not zero
    lo = pos[:, :3].min(axis=0)
    pos[:, :3] = (lo + (pos[:, :3] - lo) * 0.9).astype(pos.dtype)
    names = ("hash", "index", "dens", "dfsphAlpha", "P_l", "velAdv", "dfsphKappaV", "pres")
    for cfg in (ETA, FIXED):
        outs = []
        for flags, batched in ((0, True), (0, False), (capi.FLAG_FULL_SORT, True)):
            s = _dfsph(p, pos, vel, sc["bi"], sc["vbi"], flags=flags)
            s.dfsph_configure(*cfg)
            if batched:
                s.step(3)
                s.step(4)
            else:
                for _ in range(7):
                    s.step(1)
            outs.append(s.download(pressure=True) + tuple(s.get(x) for x in names) +
                        (s.last_iterations, s.get_stat(capi.STAT_DFSPH_DIVERGENCE_ITERATIONS)))
            if flags == 0:
                assert s.resort_stats()[0] == 6
            s.close()
        assert outs[0][2].max() > 0 and outs[0][9].max() > 0   # K and Kv are carried
        for o in outs[1:]:
            for a, b in zip(outs[0], o):
                np.testing.assert_array_equal(a, b)


def test_ignored_flags(hip_lib):
    """NRS_FLAG_FAST_ARITH and NRS_FLAG_STAGED_SCAN change nothing on a DFSPH context"""
    p, sc = small_dam_break()
    outs = []
    for flags in (0, capi.FLAG_FAST_ARITH | capi.FLAG_STAGED_SCAN):
        s = _dfsph(p, sc["pos"], _moving(sc["vel"]), sc["bi"], sc["vbi"], flags=flags)
        s.step(3)
        outs.append(s.download(pressure=True) + (s.get("dfsphKappaV"), s.last_iterations))
        s.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


def test_small_dam_break_stays_in_the_tank(hip_lib):
    p, sc = small_dam_break()
    s = _dfsph(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
    h = float(p["interactionRadius"][0])
    lo, hi = sc["bi"][:, :3].min(axis=0) - h, sc["bi"][:, :3].max(axis=0) + h
    for _ in range(4):
        s.step(50)
        pos, vel = s.download()
        assert np.all(np.isfinite(pos)) and np.all(np.isfinite(vel))
        assert np.all(pos[:, :3] >= lo) and np.all(pos[:, :3] <= hi), (pos[:, :3].min(axis=0), pos[:, :3].max(axis=0), lo, hi)
        assert s.get_stat(capi.STAT_DFSPH_DENSITY_AVG) <= 1e-3 or s.last_iterations == 100
    s.close()


def test_abi_refusals(hip_lib):
    p, pos, vel = compressed_block()
    s = _dfsph(p, pos, vel)
    nan, inf = float("nan"), float("inf")
    for args in ((-1.0, 2, 1e-3, 1, 1), (nan, 2, 1e-3, 1, 1), (inf, 2, 1e-3, 1, 1), (1e-3, 2, -1.0, 1, 1), (1e-3, 2, nan, 1, 1),
                 (1e-3, 2, inf, 1, 1), (1e-3, 0, 1e-3, 1, 1), (1e-3, 2, 1e-3, 1, 2), (1e-3, 2, 1e-3, 1, -1)):
        with pytest.raises(capi.NereusError, match="error -1"):
            s.dfsph_configure(*args)
    for call in (s.pcisph_configure, s.pbf_configure, s.pbf_set_tensile, s.pbf_set_vorticity):
        with pytest.raises(capi.NereusError, match="error -4"):
            call()
    with pytest.raises(capi.NereusError, match="error -1"):
        s.slab_configure(0, 64, 8)
    for call in (s.iisph_predict, s.iisph_iterate, s.iisph_finish):
        with pytest.raises(capi.NereusError, match="error -4"):
            call()
    for stage in (capi.STAGE_FORCES, capi.STAGE_INTEGRATE, capi.STAGE_I_DENSITY, capi.STAGE_I_SOLVE, capi.STAGE_I_INTEGRATE):
        with pytest.raises(capi.NereusError, match="error -1"):
            s.step_partial(stage)
    for stat in (capi.STAT_DENSITY_ERROR, capi.STAT_DFSPH_DENSITY_AVG, capi.STAT_DFSPH_DIVERGENCE_AVG, capi.STAT_PCISPH_DELTA,
                 capi.STAT_PBF_EPSILON):
        with pytest.raises(capi.NereusError, match="error -4"):
            s.get_stat(stat)   # no solve yet / another solver's
    assert s.get_stat(capi.STAT_DFSPH_DIVERGENCE_ITERATIONS) == 0
    for arr in ("dfsphAlpha", "dfsphKappaV", "posPred", "aii", "vorticity"):
        with pytest.raises(capi.NereusError, match="error -4"):
            s.get(arr)
    s.dfsph_configure(0.0, 1, 0.0, 0, 0)   # the ends of the ranges are accepted
    s.dfsph_configure()
    s.step(1)
    assert 2 <= s.last_iterations <= 100
    assert s.get("dfsphAlpha").shape == (len(pos),) and s.get("dfsphKappaV").shape == (len(pos),)
    with pytest.raises(capi.NereusError, match="error -4"):
        s.get("posPred")
    s.close()
    s = _dfsph(p, pos, vel)
    s.dfsph_configure(1e-3, 2, 1e-3, 0, 1)   # divergence solve off: no divergence statistic
    s.step(1)
    assert s.get_stat(capi.STAT_DFSPH_DIVERGENCE_ITERATIONS) == 0
    with pytest.raises(capi.NereusError, match="error -4"):
        s.get_stat(capi.STAT_DFSPH_DIVERGENCE_AVG)
    s.close()
    for solver in (capi.SESPH, capi.IISPH, capi.PCISPH, capi.PBF):
        o = _solver(p, pos, vel, solver=solver)
        with pytest.raises(capi.NereusError, match="error -4"):
            o.dfsph_configure()
        o.step(1)
        for arr in ("dfsphAlpha", "dfsphKappaV"):
            with pytest.raises(capi.NereusError, match="error -4"):
                o.get(arr)
        for stat in (capi.STAT_DFSPH_DENSITY_AVG, capi.STAT_DFSPH_DIVERGENCE_AVG, capi.STAT_DFSPH_DIVERGENCE_ITERATIONS):
            with pytest.raises(capi.NereusError, match="error -4"):
                o.get_stat(stat)
        o.close()
    assert hip_lib.nrs_version() == 3


def test_host_class_equals_capi(tmp_path, hip_lib):
    from tests.test_host_class import _driver, _read_out, _write_in
    p, sc = small_dam_break()
    pos, vel, bi, vbi = sc["pos"], sc["vel"], sc["bi"], sc["vbi"]
    steps = 5
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write_in(fin, pos, vel, bi, vbi)
    subprocess.check_call([_driver(), "run", "dfsph", fin, str(steps), fout], stdout=subprocess.DEVNULL)
    got = _read_out(fout)
    s = _dfsph(Oracle.default_params(SESPH), pos, vel, bi, vbi)
    for _ in range(steps):
        s.step(1)
    gp, gv, gpr = s.download(pressure=True)
    np.testing.assert_array_equal(got["pos"], gp)
    np.testing.assert_array_equal(got["vel"], gv)
    np.testing.assert_array_equal(got["pressure"], gpr)
    assert got["iters"] == s.last_iterations > 0
    s.close()


def test_c3_one_step(hip_lib):
    """BASELINE config C3 (160^3 = 4,096,000 particles, fp32) with the IISPH constructor's parameters and the default settings"""
    p = Oracle.default_params(IISPH)
    sc = scene.dam_break("C3", h=float(p["interactionRadius"][0]), kpoly=float(p["kpoly"][0]))
    assert len(sc["pos"]) == 4_096_000
    s = _dfsph(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
    s.step(1)
    pos, vel = s.download()
    assert np.all(np.isfinite(pos)) and np.all(np.isfinite(vel))
    avg = s.get_stat(capi.STAT_DFSPH_DENSITY_AVG)
    assert avg <= 1e-3 or s.last_iterations == 100, (avg, s.last_iterations)
    assert s.get_stat(capi.STAT_DFSPH_DIVERGENCE_ITERATIONS) >= 1
    s.close()
