"""The PBF tensile correction and vorticity confinement on the device: list-driven against reference-order kernels bit for bit, the
device against the float64 model (tests/pbf_extras_model.py), "off" exactly as before, the physics checks of the model on the device,
the refusals of the ABI, the host class and one step at config C3."""
import subprocess

import numpy as np
import pytest

from nereus_amd import capi, scene
from tests import pbf_extras_model as M
from tests.common import rel_err, small_dam_break
from tests.oracle_lib import IISPH, SESPH, Oracle
from tests.test_pcisph_gpu import _bitwise_scenes, _solver

pytestmark = pytest.mark.gpu

K, DQ, EPS_V = 1e-3, 0.3, 0.5   # large enough that both terms move the bits of every scene


def _pbf(p, pos, vel, bi=None, vbi=None, **kw):
    return _solver(p, pos, vel, bi, vbi, solver=capi.PBF, **kw)


@pytest.mark.parametrize("xsph", [0.0, 0.1])
def test_list_kernels_equal_reference_order_bitwise(hip_lib, xsph):
    """The four scenes of the PCISPH test (two of them overflow their hit lists) with s_corr and confinement on: at P_SOLVE (fixed 3
    iterations) and after three full steps, the vorticity included."""
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
            s.pbf_configure(0.0, 3, 0.01, xsph)
            s.pbf_set_tensile(K, DQ)
            s.pbf_set_vorticity(EPS_V)
            s.step_partial(capi.STAGE_P_SOLVE)
            got = [s.get(nm) for nm in solve]
            s.set_particles(pos, vel)
            s.step(3)
            got += list(s.download(pressure=True)) + [s.get("vorticity")]
            outs.append(got)
            s.close()
        assert np.any(outs[0][-1][:, 3] > 0)
        for nm, a, b in zip(solve + ["pos", "vel", "pressure", "vorticity"], *outs):
            np.testing.assert_array_equal(a, b, err_msg="scene %d %s" % (k, nm))


def _advected_dam(double, kernel_set=capi.MULLER):
    """the small dam break squeezed to 0.87 (as tests/test_pcisph_gpu.py's _scenes: the particles along the floor and the walls are
    compressed) and set swirling about z, after 3 plain PBF steps: a moving state without the symmetry of the lattice that is still
    compressed enough for lambda to be well above fp32 roundoff (C = rho* / rho0 - 1 cancels).  Monaghan (tests/test_pcisph_gpu.py
    _monaghan_scenes): squeezed to 0.65, time step 2e-4, and no plain steps — its loop relaxes the compression within them; the
    jittered lattice has no exact symmetry either."""
    p, sc = small_dam_break(double=double, kernel_set=kernel_set)
    mon = kernel_set == capi.MONAGHAN
    if mon:
        p["timestep"] = 2e-4
    pos = sc["pos"].copy()
    lo = pos[:, :3].min(axis=0)
    pos[:, :3] = (lo + (pos[:, :3] - lo) * (0.65 if mon else 0.87)).astype(pos.dtype)
    vel = np.zeros_like(pos)
    vel[:, :3] = np.cross([0.0, 0.0, 5.0], pos[:, :3] - pos[:, :3].mean(axis=0))
    if mon:
        return p, pos, vel, sc["bi"], sc["vbi"]
    s = _pbf(p, pos, vel, sc["bi"], sc["vbi"], double=double, kernel_set=kernel_set)
    s.step(3)
    pos, vel = s.download()
    s.close()
    return p, pos, vel, sc["bi"], sc["vbi"]


@pytest.mark.parametrize("double,tol", [(False, 1e-4), (True, 1e-10)])
@pytest.mark.parametrize("ref", [False, True])
@pytest.mark.parametrize("iters", [1, 3])
def test_device_matches_model(hip_lib, double, tol, ref, iters):
    _device_matches_model(double, tol, ref, iters, capi.MULLER)


@pytest.mark.parametrize("double,tol", [(False, 1e-4), (True, 1e-10)])
@pytest.mark.parametrize("ref", [False, True])
@pytest.mark.parametrize("iters", [1, 3])
def test_monaghan_device_matches_model(hip_lib, double, tol, ref, iters):
    """test_device_matches_model with the Monaghan kernels: W, W_q and the gradient of lambda, s_corr, omega and eta are the Monaghan
    branch, against the model's Monaghan restatement; the context builds no hit lists."""
    _device_matches_model(double, tol, ref, iters, capi.MONAGHAN)


def _device_matches_model(double, tol, ref, iters, kernel_set):
    eps_v = 2.0 if kernel_set == capi.MULLER else 10.0   # a kick well above the velocity tolerance (Monaghan: dt is 1 / 5)
    p, pos, vel, bi, vbi = _advected_dam(double, kernel_set)
    xsph = 0.1 if iters == 3 else 0.0
    s = _pbf(p, pos, vel, bi, vbi, double=double, reference_order=ref, kernel_set=kernel_set)
    s.pbf_configure(0.0, iters, 0.01, xsph)
    s.pbf_set_tensile(K, DQ)
    s.pbf_set_vorticity(eps_v)
    s.step_partial(capi.STAGE_P_ADVECT)
    x, va, bs = s.get("sortedPos"), s.get("velAdv"), s.get("bSorted")
    s.set_particles(pos, vel)
    s.step_partial(capi.STAGE_P_SOLVE)
    dev = {nm: s.get(nm) for nm in ("P_l", "posPred")}
    eps = s.get_stat(capi.STAT_PBF_EPSILON)
    s.set_particles(pos, vel)
    s.step(1)
    dev["pos"], dev["vel"] = s.download()
    dev["omega"] = s.get("vorticity")
    if kernel_set == capi.MONAGHAN:
        with pytest.raises(capi.NereusError, match="error -4"):
            s.get_stat(capi.STAT_HIT_MEAN)
    s.close()
    np.testing.assert_allclose(eps, 0.01 * M.prototype_d(p, kernel_set)[0], rtol=1e-5)
    m = M.run(p, x, va, bs[:, :3], bs[:, 3], eps=eps, min_iters=iters, eta=0.0, xsph=xsph, k=K, dq=DQ, eps_v=eps_v, kernel_set=kernel_set)
    plain = M.run(p, x, va, bs[:, :3], bs[:, 3], eps=eps, min_iters=iters, eta=0.0, xsph=xsph, kernel_set=kernel_set)
    assert rel_err(m["xs"] - plain["xs"], np.zeros_like(m["xs"])) > 0   # s_corr moves x*
    assert m["lam"].min() < 0
    assert rel_err(dev["P_l"], m["lam"]) <= tol
    assert rel_err(dev["posPred"][:, :3], m["xs"]) <= tol
    assert rel_err(dev["pos"][:, :3], m["pos"]) <= tol
    np.testing.assert_array_equal(dev["pos"][:, :3], dev["posPred"][:, :3])
    # omega differences velocities (x* - x) / dt of neighbours: 10x the velocity tolerance of tests/test_pbf_gpu.py
    assert rel_err(dev["omega"][:, :3], m["omega"]) <= 100 * tol, rel_err(dev["omega"][:, :3], m["omega"])
    # Particles whose |eta| lies within a factor 2 of the cut 1e-3 |omega| / h are left out: there, roundoff decides whether N is
    # set, and with it whether the particle gets its kick.
    h = float(p["interactionRadius"][0])
    cut = M.VORT_CUT * np.linalg.norm(m["omega"], axis=1) / h
    en = np.linalg.norm(m["eta_v"], axis=1)
    keep = ~((en > 0.5 * cut) & (en < 2 * cut))
    assert np.count_nonzero(keep) >= 0.9 * len(keep)
    assert np.count_nonzero(np.any(m["N"][keep] != 0, axis=1)) > 0.5 * np.count_nonzero(keep)   # most particles get a kick
    assert rel_err(dev["vel"][keep, :3], m["vel"][keep]) <= 10 * tol, rel_err(dev["vel"][keep, :3], m["vel"][keep])
    kick = m["vel"] - plain["vel"]
    assert np.max(np.abs(kick[keep])) > 5e-3 * np.max(np.abs(m["vel"]))   # above the velocity tolerance of both precisions


def test_off_means_unchanged(hip_lib):
    """k = 0 and eps_v = 0 set explicitly (also after having been on) give the bits of a context that never called the setters, with
    the same launches per stage."""
    p, sc = small_dam_break()
    outs, launches = [], []
    for mode in ("never", "zero", "back"):
        s = _pbf(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
        s.pbf_configure(0.01, 2, 0.01, 0.1)
        if mode == "zero":
            s.pbf_set_tensile(0.0, 0.2)
            s.pbf_set_vorticity(0.0)
        if mode == "back":
            s.pbf_set_tensile(K, 0.5)
            s.pbf_set_vorticity(EPS_V)
            s.pbf_set_tensile(0.0, 0.2)
            s.pbf_set_vorticity(0.0)
        s.set_profiling(True)
        s.step(5)
        st = s.stage_ms()
        launches.append([st[nm][1] for nm in ("p_solve", "p_integrate")])
        outs.append(list(s.download(pressure=True)) + [s.get("posPred"), np.array([s.last_iterations])])
        if mode == "never":
            with pytest.raises(capi.NereusError, match="error -4"):
                s.get("vorticity")   # no step with confinement yet
        s.close()
    for o, l in zip(outs[1:], launches[1:]):
        assert l == launches[0]
        for a, b in zip(outs[0], o):
            np.testing.assert_array_equal(a, b)


def test_tensile_pair_separates_as_in_model(hip_lib):
    p = Oracle.default_params(IISPH)
    h = float(p["interactionRadius"][0])
    pos = np.ones((2, 4), np.float32)
    pos[:, :3] = [[0.1, 0.1, 0.1], [0.1 + 0.8 * h, 0.1, 0.1]]
    vel = np.zeros_like(pos)
    got = {}
    for k in (0.0, 1e-3):
        s = _pbf(p, pos, vel)
        s.pbf_configure(0.0, 2)
        s.pbf_set_tensile(k, 0.7)
        s.step_partial(capi.STAGE_P_ADVECT)
        x, va = s.get("sortedPos"), s.get("velAdv")
        x0 = s.get("posPred")[:, :3].astype(np.float64)
        s.set_particles(pos, vel)
        s.step_partial(capi.STAGE_P_SOLVE)
        xs, lam = s.get("posPred")[:, :3].astype(np.float64), s.get("P_l")
        s.close()
        m = M.run(p, x, va, min_iters=2, eta=0.0, k=k, dq=0.7)
        assert np.all(lam == 0) and np.all(m["lam"] == 0)
        sep = abs(xs[1, 0] - xs[0, 0]) - abs(x0[1, 0] - x0[0, 0])   # (in either sorted order)
        msep = abs(m["xs"][1, 0] - m["xs"][0, 0]) - abs(x0[1, 0] - x0[0, 0])
        got[k] = (sep, msep, xs, x0)
    assert np.array_equal(got[0.0][2], got[0.0][3])   # no s_corr: x* does not move
    sep, msep = got[1e-3][:2]
    assert msep > 2e-4 and abs(sep - msep) <= 1e-3 * msep, (sep, msep)
    d = got[1e-3][2] - got[1e-3][3]
    assert np.all(np.abs(d[:, 1:]) <= 1e-7)   # along the axis


def _rotating_block(eps_v):
    p = Oracle.default_params(IISPH)
    p["gravity"] = 0
    m, rd = float(p["particleMass"][0]), float(p["restDensity"][0])
    s_ = float(np.cbrt(m / rd))
    g = np.stack(np.meshgrid(*(np.arange(10),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    pos = np.ones((len(g), 4), np.float32)
    pos[:, :3] = (g - 4.5) * s_
    vel = np.zeros_like(pos)
    vel[:, :3] = np.cross([0.0, 0.0, 5.0], pos[:, :3])
    s = _pbf(p, pos, vel)
    s.pbf_configure(0.01, 2, 0.01, 0.1)
    s.pbf_set_vorticity(eps_v)
    s.step(20)
    x, v = (a.astype(np.float64) for a in s.download())
    s.close()
    c = x[:, :3].mean(axis=0)
    return float(np.sum(m * np.cross(x[:, :3] - c, v[:, :3])[:, 2])), x, v


def test_confinement_keeps_a_rotating_block_spinning(hip_lib):
    """No gravity, no boundaries, XSPH 0.1, 20 steps: the block keeps more angular momentum with confinement than without."""
    l0, x0, v0 = _rotating_block(0.0)
    l1, x1, v1 = _rotating_block(1.0)
    assert np.all(np.isfinite(x1)) and np.all(np.isfinite(v1))
    assert l0 > 0 and l1 > l0 * (1 + 1e-3), (l0, l1)


def test_abi_refusals(hip_lib):
    p, sc = small_dam_break()
    s = _pbf(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
    nan, inf = float("nan"), float("inf")
    for args in ((-1e-3, 0.2), (nan, 0.2), (inf, 0.2), (1e-3, 0.0), (1e-3, 1.0), (1e-3, -0.1), (1e-3, nan), (1e-3, inf)):
        with pytest.raises(capi.NereusError, match="error -1"):
            s.pbf_set_tensile(*args)
    for e in (-0.1, nan, inf):
        with pytest.raises(capi.NereusError, match="error -1"):
            s.pbf_set_vorticity(e)
    with pytest.raises(capi.NereusError, match="error -4"):
        s.get("vorticity")
    s.pbf_set_tensile(0.0, 0.2)   # the defaults, and the ends of the ranges, are accepted
    s.pbf_set_tensile(1.0, 0.999)
    s.pbf_set_tensile(1e-4, 1e-3)
    s.pbf_set_vorticity(0.0)
    s.pbf_set_vorticity(0.01)
    s.step(1)
    assert s.get("vorticity").shape == (len(sc["pos"]), 4)
    s.close()
    for solver in (capi.SESPH, capi.IISPH, capi.PCISPH):
        o = _solver(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"], solver=solver)
        with pytest.raises(capi.NereusError, match="error -4"):
            o.pbf_set_tensile(1e-3, 0.2)
        with pytest.raises(capi.NereusError, match="error -4"):
            o.pbf_set_vorticity(0.01)
        o.step(1)
        with pytest.raises(capi.NereusError, match="error -4"):
            o.get("vorticity")
        o.close()
    assert hip_lib.nrs_version() == 3


def test_host_class_pbf_full_equals_capi(tmp_path, hip_lib):
    """headless run pbf-full: XSPH 0.01, k = 1e-4, dq = 0.2, eps_v = 0.01 (the host class hands over SReal values)"""
    from tests.test_host_class import _driver, _read_out, _write_in
    p, sc = small_dam_break()
    pos, vel, bi, vbi = sc["pos"], sc["vel"], sc["bi"], sc["vbi"]
    steps = 5
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write_in(fin, pos, vel, bi, vbi)
    subprocess.check_call([_driver(), "run", "pbf-full", fin, str(steps), fout], stdout=subprocess.DEVNULL)
    got = _read_out(fout)
    f = lambda v: float(np.float32(v))   # noqa: E731
    s = _pbf(Oracle.default_params(SESPH), pos, vel, bi, vbi)
    s.pbf_configure(f(0.01), 2, f(0.01), f(0.01))
    s.pbf_set_tensile(f(1e-4), f(0.2))
    s.pbf_set_vorticity(f(0.01))
    for _ in range(steps):
        s.step(1)
    gp, gv, gpr = s.download(pressure=True)
    np.testing.assert_array_equal(got["pos"], gp)
    np.testing.assert_array_equal(got["vel"], gv)
    np.testing.assert_array_equal(got["pressure"], gpr)
    assert got["iters"] == s.last_iterations > 0
    s.close()


def test_c3_one_step_with_both_terms(hip_lib):
    """BASELINE config C3 (160^3 = 4,096,000 particles, fp32) with the IISPH constructor's parameters, s_corr and confinement on"""
    p = Oracle.default_params(IISPH)
    sc = scene.dam_break("C3", h=float(p["interactionRadius"][0]), kpoly=float(p["kpoly"][0]))
    assert len(sc["pos"]) == 4_096_000
    s = _pbf(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
    s.pbf_configure(0.01, 2, 0.01, 0.01)
    s.pbf_set_tensile(1e-4, 0.2)
    s.pbf_set_vorticity(0.01)
    s.step(1)
    pos, vel = s.download()
    assert np.all(np.isfinite(pos)) and np.all(np.isfinite(vel))
    h = float(p["interactionRadius"][0])
    lo, hi = sc["bi"][:, :3].min(axis=0) - h, sc["bi"][:, :3].max(axis=0) + h
    assert np.all(pos[:, :3] >= lo) and np.all(pos[:, :3] <= hi)
    s.close()
