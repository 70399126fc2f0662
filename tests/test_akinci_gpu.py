"""Akinci surface tension and wall adhesion on the device (nrs_set_surface_akinci; PCISPH, PBF, DFSPH): the two kernels against the
reference's own outputs, list-driven against reference-order kernels bit for bit, the device against the float64 model
(tests/akinci_model.py), "off" exactly as before, the physics checks, the refusals of the ABI, the host class and one step at config C3."""
import subprocess

import numpy as np
import pytest

from nereus_amd import capi, scene
from tests import akinci_model as M
from tests import ref_pin
from tests.common import rel_err, small_dam_break
from tests.oracle_lib import IISPH, SESPH, Oracle
from tests.test_akinci_cpu import GOLD, random_blob
from tests.test_pbf_extras_gpu import _advected_dam
from tests.test_pcisph_gpu import _bitwise_scenes, _solver

pytestmark = pytest.mark.gpu

GAMMA, BETA = 1.0, 1.0   # forces of the order of the particle's weight on the tests' scenes: they move the bits of every scene
# test_device_matches_model: the walls of the squeezed dam push with hundreds of times a particle's weight, and the bars are relative to
# the largest force, so the coefficients are raised until each of the three terms stands 100 x above the tolerance (only the
# advection stage is evaluated there, nothing is stepped)
MODEL_GAMMA, MODEL_BETA = 300.0, 1500.0
SOLVERS = [capi.PCISPH, capi.PBF, capi.DFSPH]
NAMES = {capi.PCISPH: "pcisph", capi.PBF: "pbf", capi.DFSPH: "dfsph"}


@pytest.mark.parametrize("double", [0, 1])
def test_device_akinci_kernels_equal_reference_fixture(hip_lib, double):
    """nrs_eval_smoothing which = 6 / 7 against the outputs of the reference's own header (committed fixture).  Cakinci: bit for bit.
    Aboundary: NaN exactly where the fixture has NaN, exact zeros out of branch, otherwise within 2 * 2^-23 relative — two faithful
    powf implementations differ by at most one float ulp (2^-23 relative at most), and the product with bpol rounds once more."""
    g = np.load(GOLD)
    nans = 0
    for hi, h in enumerate(g["radii"]):
        tag = "d%d_h%d" % (double, hi)
        r = np.ascontiguousarray(g[tag + "_r"])
        c0, c1 = ref_pin.constants(6, float(h), double)
        want = np.ascontiguousarray(g[tag + "_f6"])
        got = capi.eval_smoothing(6, r, None, float(h), c0, c1, bool(double))
        np.testing.assert_array_equal(ref_pin.bits(got), ref_pin.bits(want), err_msg="Cakinci d=%d h=%g" % (double, h))
        assert np.count_nonzero(want[:, 0]) > 100
        c0, c1 = ref_pin.constants(7, float(h), double)
        want = g[tag + "_f7"][:, 0].astype(np.float64)
        got = capi.eval_smoothing(7, r, None, float(h), c0, c1, bool(double))[:, 0].astype(np.float64)
        ln = M._len(r).astype(np.float64)
        out = ~((2.0 * ln > float(r.dtype.type(h))) & (ln <= float(r.dtype.type(h))))
        assert np.all(want[out] == 0) and np.all(got[out] == 0)
        nan = np.isnan(want)
        nans += int(nan.sum())
        assert np.array_equal(np.isnan(got), nan), "Aboundary d=%d h=%g: NaN sites differ" % (double, h)
        ok = ~nan & ~out
        assert np.count_nonzero(ok) > 100
        diff, bound = np.abs(got[ok] - want[ok]), 2 * 2.0 ** -23 * np.abs(want[ok])   # (in-branch values may be exactly 0: r = h)
        nz = want[ok] != 0
        print("Aboundary d=%d h=%g: max relative difference %.3g (bound %.3g)" % (double, h, np.max(diff[nz] / np.abs(want[ok][nz])), 2 * 2.0 ** -23))
        assert np.all(diff <= bound)
    assert double or nans > 0   # (the fp32 fixture holds NaN sites)


def _configure(s, solver):
    if solver == capi.PBF:
        s.pbf_configure(0.01, 2, 0.01, 0.1)


@pytest.mark.parametrize("solver", SOLVERS)
def test_list_kernels_equal_reference_order_bitwise(hip_lib, solver):
    """The four scenes of the PCISPH test (two of them overflow their hit lists) with both terms on: the normals and the advection
    stage's results at P_ADVECT, and the state after three full steps."""
    adv = ["normals", "forcesAdv", "velAdv"] + ([] if solver == capi.DFSPH else ["posPred"])   # (a DFSPH context refuses posPred)
    for k, (pp, pos, vel, bi, vbi, overflows) in enumerate(_bitwise_scenes()):
        if overflows:
            s = _solver(pp, pos, vel, bi, vbi, solver=solver)
            s.step(1)
            assert s.get_stat(capi.STAT_HIT_OVERFLOW) > 0   # the scene really takes the per-particle fallback
            s.close()
        s = _solver(pp, pos, vel, bi, vbi, solver=solver)
        _configure(s, solver)
        s.step_partial(capi.STAGE_P_ADVECT)
        off = s.get("forcesAdv")
        s.close()
        outs = []
        for ref in (False, True):
            s = _solver(pp, pos, vel, bi, vbi, solver=solver, reference_order=ref)
            _configure(s, solver)
            s.surface_akinci(GAMMA, BETA)
            s.step_partial(capi.STAGE_P_ADVECT)
            got = [s.get(nm) for nm in adv]
            s.set_particles(pos, vel)
            s.step(3)
            got += list(s.download(pressure=True))
            outs.append(got)
            s.close()
        assert np.any(outs[0][1] != off), "scene %d: the model does not move forcesAdv" % k
        assert np.any(outs[0][0][:, :3] != 0)
        for nm, a, b in zip(adv + ["pos", "vel", "pressure"], *outs):
            np.testing.assert_array_equal(a, b, err_msg="%s scene %d %s" % (NAMES[solver], k, nm))


@pytest.mark.parametrize("double,tol", [(False, 1e-4), (True, 1e-10)])
@pytest.mark.parametrize("kernel_set", [capi.MULLER, capi.MONAGHAN])
@pytest.mark.parametrize("ref", [False, True])
def test_device_matches_model(hip_lib, double, tol, kernel_set, ref):
    """The advected, squeezed dam of the PBF extras test at P_ADVECT: the normals against the model, and forcesAdv against the
    forcesAdv of a context with the model off and without the reference-style cohesion (which gamma > 0 leaves out) plus the model's
    F^coh + F^curv + F^adh.  Each of the three terms is at least 100 x the tolerance of the force scale, so none of them can pass as
    zero."""
    p, pos, vel, bi, vbi = _advected_dam(double, kernel_set)
    kw = dict(solver=capi.PBF, double=double, kernel_set=kernel_set, reference_order=ref)
    s = _solver(p, pos, vel, bi, vbi, **kw)
    s.surface_akinci(MODEL_GAMMA, MODEL_BETA)
    s.step_partial(capi.STAGE_P_ADVECT)
    x, rho, bs, nrm, fa = (s.get(nm) for nm in ("sortedPos", "dens", "bSorted", "normals", "forcesAdv"))
    s.close()
    s = _solver(p, pos, vel, bi, vbi, surface_tension=False, **kw)
    s.step_partial(capi.STAGE_P_ADVECT)
    base = s.get("forcesAdv")
    s.close()
    m = M.run(p, x, rho, MODEL_GAMMA, MODEL_BETA, bs[:, :3], bs[:, 3], kernel_set=kernel_set)
    np.testing.assert_array_equal(nrm[:, 3], rho)
    want = base[:, :3].astype(np.float64) + m["f"]
    scale = np.max(np.abs(want))
    parts = {k: float(np.max(np.abs(m[k])) / scale) for k in ("coh", "curv", "adh")}
    en, ef = rel_err(nrm[:, :3], m["n"]), rel_err(fa[:, :3], want)
    print("double=%d kernel_set=%d ref=%d: normals %.3g forcesAdv %.3g (tol %.0e); terms / force scale %s; off-run differs by %.3g"
          % (double, kernel_set, ref, en, ef, tol, parts, rel_err(base[:, :3], want)))
    assert min(parts.values()) >= 100 * tol, parts
    assert rel_err(base[:, :3], want) >= 100 * tol   # the run with gamma = beta_a = 0 is far outside the tolerance
    assert en <= tol, en
    assert ef <= tol, ef
    assert np.all(fa[:, 3] == 0)


@pytest.mark.parametrize("solver", SOLVERS)
def test_off_means_unchanged(hip_lib, solver):
    """Never set, set to (0, 0), and switched on and back to (0, 0): the same bits after 5 steps and the same launches per stage."""
    p, sc = small_dam_break()
    outs, launches = [], []
    for mode in ("never", "zero", "back"):
        s = _solver(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"], solver=solver)
        _configure(s, solver)
        if mode == "zero":
            s.surface_akinci(0.0, 0.0)
        if mode == "back":
            s.surface_akinci(GAMMA, BETA)
            s.surface_akinci(0.0, 0.0)
        s.set_profiling(True)
        s.step(5)
        st = s.stage_ms()
        launches.append({nm: v[1] for nm, v in st.items()})
        outs.append(list(s.download(pressure=True)) + [s.get("forcesAdv"), s.get("velAdv"), np.array([s.last_iterations])])
        with pytest.raises(capi.NereusError, match="error -4"):
            s.get("normals")   # no step with gamma > 0
        s.close()
    assert launches[0]["p_advect"] > 0
    for o, l in zip(outs[1:], launches[1:]):
        assert l == launches[0]
        for a, b in zip(outs[0], o):
            np.testing.assert_array_equal(a, b)


def test_blob_forces_sum_to_zero_fp64(hip_lib):
    """The random blob of the CPU test, fp64, no gravity, no boundaries, zero velocities: forcesAdv is F^coh + F^curv alone, and its
    sum over the particles is within the CPU bar |sum F| <= 1e-10 sum |F_i| (exactly antisymmetric pair terms, N eps of roundoff)."""
    p, x = random_blob()
    p["gravity"] = 0
    pos = np.ones((len(x), 4))
    pos[:, :3] = x
    for ref in (False, True):
        s = _solver(p, pos, np.zeros_like(pos), solver=capi.PBF, double=True, reference_order=ref)
        s.surface_akinci(GAMMA, 0.0)
        s.step_partial(capi.STAGE_P_ADVECT)
        f, xs, rho = s.get("forcesAdv")[:, :3], s.get("sortedPos"), s.get("dens")
        s.close()
        per = np.linalg.norm(f, axis=1)
        total = np.linalg.norm(f.sum(axis=0))
        print("ref=%d: |sum F| = %.3g, sum |F_i| = %.3g, ratio %.3g" % (ref, total, per.sum(), total / per.sum()))
        assert per.max() > 0 and total <= 1e-10 * per.sum()
        m = M.run(p, xs, rho, GAMMA, 0.0)
        assert rel_err(f, m["f"]) <= 1e-10


# Measured on the MI355X, largest distance from the centroid (start 0.332203 m) after 20 steps with gamma = 0 / 0.5 / 1 / 2:
# PBF 0.332556 / 0.329992 / 0.330133 / 0.330217, DFSPH 0.340524 / 0.339441 / 0.339007 / 0.338027 — a gap of 2.4 mm (PBF) and 1.5 mm
# (DFSPH) at gamma = 1.  (The lattice at rest spacing has six neighbours per particle and swells under the pressure solve alone; after
# 40 and 80 steps DFSPH keeps the sign for every gamma, gaps of 3.4 - 6.0 mm, while PBF's corners oscillate: 0.336290 / 0.335529 /
# 0.337866 / 0.334650 at 40 steps.)  The margin is a third of the smaller gap.
CUBE_STEPS, CUBE_GAMMA, CUBE_MARGIN = 20, 1.0, 5e-4


def _free_cube(solver, gamma):
    p = Oracle.default_params(IISPH)
    p["gravity"] = 0
    m, rd = float(p["particleMass"][0]), float(p["restDensity"][0])
    sp = float(np.cbrt(m / rd))
    g = np.stack(np.meshgrid(*(np.arange(10),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    pos = np.ones((len(g), 4), np.float32)
    pos[:, :3] = (g - 4.5) * sp
    s = _solver(p, pos, np.zeros_like(pos), solver=solver)
    s.surface_akinci(gamma, 0.0)
    s.step(CUBE_STEPS)
    x, v = (a.astype(np.float64) for a in s.download())
    s.close()
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(v))
    return float(np.max(np.linalg.norm(x[:, :3] - x[:, :3].mean(axis=0), axis=1))), 4.5 * sp * np.sqrt(3.0)


@pytest.mark.parametrize("solver", [capi.PBF, capi.DFSPH])
def test_free_cube_rounds_off(hip_lib, solver):
    """A free 10^3 cube at rest spacing, zero gravity, no boundaries, 20 steps: surface tension pulls the corners in.  Measured: PBF
    0.332556 m without and 0.330133 m with gamma = 1, DFSPH 0.340524 m and 0.339007 m; asserted: 0.5 mm."""
    r0, start = _free_cube(solver, 0.0)
    r1, _ = _free_cube(solver, CUBE_GAMMA)
    print("%s: corner distance start %.6f, after %d steps gamma=0 %.6f, gamma=%g %.6f, gap %.6f"
          % (NAMES[solver], start, CUBE_STEPS, r0, CUBE_GAMMA, r1, r0 - r1))
    assert r1 < r0 - CUBE_MARGIN, (r0, r1)


def test_wall_adhesion_points_at_the_wall(hip_lib):
    """Particles at 0.6 h, 0.75 h and 0.9 h above the sampled floor of the small tank (far from its side walls and from each other)
    and one at 3 h, zero gravity, zero velocity: forcesAdv with beta_a on minus forcesAdv with it off points at the floor (within 45
    degrees of its normal) for the three, and is exactly zero for the fourth."""
    p, sc = small_dam_break()
    p["gravity"] = 0
    h = float(p["interactionRadius"][0])
    tank = sc["tank"]
    heights = np.array([0.6, 0.75, 0.9, 3.0]) * h
    pos = np.ones((4, 4), np.float32)
    pos[:, 0] = 0.5 * tank[0] + 3.1 * h * np.arange(4) + 0.003
    pos[:, 1] = heights
    pos[:, 2] = 0.5 * tank[2] + 0.007
    d = np.linalg.norm(pos[:, None, :3].astype(np.float64) - sc["bi"][None, :, :3], axis=2).min(axis=1)
    assert np.all((d[:3] > 0.5 * h) & (d[:3] < h)) and d[3] > h
    for solver in SOLVERS:
        for ref in (False, True):
            f = {}
            for beta in (0.0, BETA):
                s = _solver(p, pos, np.zeros_like(pos), sc["bi"], sc["vbi"], solver=solver, reference_order=ref)
                s.surface_akinci(0.0, beta)
                s.step_partial(capi.STAGE_P_ADVECT)
                f[beta], xs = s.get("forcesAdv")[:, :3].astype(np.float64), s.get("sortedPos")
                s.close()
            diff = f[BETA] - f[0.0]
            near = xs[:, 1] < 2 * h
            assert near.sum() == 3
            assert np.all(diff[near, 1] < 0), diff
            assert np.all(np.hypot(diff[near, 0], diff[near, 2]) <= -diff[near, 1]), diff
            assert np.all(diff[~near] == 0), diff


def test_abi_refusals(hip_lib):
    p, sc = small_dam_break()
    nan, inf = float("nan"), float("inf")
    for solver in SOLVERS:
        s = _solver(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"], solver=solver)
        for args in ((-1.0, 0.0), (0.0, -1.0), (nan, 0.0), (0.0, nan), (inf, 0.0), (0.0, inf)):
            with pytest.raises(capi.NereusError, match="error -1"):
                s.surface_akinci(*args)
        with pytest.raises(capi.NereusError, match="error -4"):
            s.get("normals")
        s.surface_akinci(0.0, BETA)   # adhesion alone forms no normals
        s.step(1)
        with pytest.raises(capi.NereusError, match="error -4"):
            s.get("normals")
        s.surface_akinci(GAMMA, 0.0)
        s.step(1)
        assert s.get("normals").shape == (len(sc["pos"]), 4)
        s.close()
    for solver in (capi.SESPH, capi.IISPH):
        o = _solver(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"], solver=solver)
        with pytest.raises(capi.NereusError, match="error -4"):
            o.surface_akinci(GAMMA, BETA)
        with pytest.raises(capi.NereusError, match="error -4"):
            o.surface_akinci(0.0, 0.0)
        o.step(1)
        with pytest.raises(capi.NereusError, match="error -4"):
            o.get("normals")
        o.close()
    assert hip_lib.nrs_version() == 3


def test_host_class_dfsph_akinci_equals_capi(tmp_path, hip_lib):
    """headless run dfsph-akinci: Nereus::DFSPH with setAkinciSurface(1, 1)"""
    from tests.test_host_class import _driver, _read_out, _write_in
    p, sc = small_dam_break()
    pos, vel, bi, vbi = sc["pos"], sc["vel"], sc["bi"], sc["vbi"]
    steps = 5
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write_in(fin, pos, vel, bi, vbi)
    subprocess.check_call([_driver(), "run", "dfsph-akinci", fin, str(steps), fout], stdout=subprocess.DEVNULL)
    got = _read_out(fout)
    s = _solver(Oracle.default_params(SESPH), pos, vel, bi, vbi, solver=capi.DFSPH)
    s.surface_akinci(1.0, 1.0)
    for _ in range(steps):
        s.step(1)
    gp, gv, gpr = s.download(pressure=True)
    np.testing.assert_array_equal(got["pos"], gp)
    np.testing.assert_array_equal(got["vel"], gv)
    np.testing.assert_array_equal(got["pressure"], gpr)
    assert got["iters"] == s.last_iterations > 0
    plain = _solver(Oracle.default_params(SESPH), pos, vel, bi, vbi, solver=capi.DFSPH)
    plain.step(steps)
    assert np.any(plain.download()[0] != gp)   # the run mode really switches the model on
    plain.close()
    s.close()


def test_c3_one_dfsph_step_with_both_terms(hip_lib):
    """BASELINE config C3 (160^3 = 4,096,000 particles, fp32) with the IISPH constructor's parameters, surface tension and adhesion on"""
    p = Oracle.default_params(IISPH)
    sc = scene.dam_break("C3", h=float(p["interactionRadius"][0]), kpoly=float(p["kpoly"][0]))
    assert len(sc["pos"]) == 4_096_000
    s = _solver(p, sc["pos"], sc["vel"], sc["bi"], sc["vbi"], solver=capi.DFSPH)
    s.surface_akinci(GAMMA, BETA)
    s.step(1)
    pos, vel = s.download()
    assert np.all(np.isfinite(pos)) and np.all(np.isfinite(vel))
    assert np.all(np.isfinite(s.get("normals")))
    h = float(p["interactionRadius"][0])
    lo, hi = sc["bi"][:, :3].min(axis=0) - h, sc["bi"][:, :3].max(axis=0) + h
    assert np.all(pos[:, :3] >= lo) and np.all(pos[:, :3] <= hi)
    s.close()
