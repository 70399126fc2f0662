"""PCISPH and PBF at the edge sizes, on both kernel paths, against the float64 models (tests/pcisph_model.py, tests/pbf_model.py): an
empty context (the step is a no-op), one particle, ragged counts around the 64-lane wave and the 256-thread block, a scene with walls,
and particles appended between steps (the next step equals a fresh context loaded with the concatenated state, bit for bit)."""
import numpy as np
import pytest

from nereus_amd import capi
from tests import pbf_model, pcisph_model
from tests.common import compressed_block, rel_err, small_dam_break
from tests.test_pcisph_gpu import _solver

pytestmark = pytest.mark.gpu

SOLVERS = [capi.PCISPH, capi.PBF]


def _configure(s, solver, iters):
    if solver == capi.PCISPH:
        s.pcisph_configure(0.01, iters)
        s.set_max_iterations(iters)
    else:
        s.pbf_configure(0.0, iters, 0.01, 0.1)


def _device_and_model(p, pos, vel, bi, vbi, solver, ref, iters=3):
    """the solve stage and one step on the device; the model from the device's sorted start state"""
    s = _solver(p, pos, vel, bi, vbi, solver=solver, reference_order=ref)
    _configure(s, solver, iters)
    s.step_partial(capi.STAGE_P_ADVECT)
    x, va = s.get("sortedPos"), s.get("velAdv")
    bs = s.get("bSorted") if bi is not None else None
    s.set_particles(pos, vel)
    s.step_partial(capi.STAGE_P_SOLVE)
    dev = {nm: s.get(nm) for nm in ("densCorr", "P_l", "forcesP", "posPred")}
    dev["iters"] = s.last_iterations
    stat = s.get_stat(capi.STAT_PCISPH_DELTA if solver == capi.PCISPH else capi.STAT_PBF_EPSILON)
    s.set_particles(pos, vel)
    s.step(1)
    dev["pos"], dev["vel"], dev["pressure"] = s.download(pressure=True)
    s.close()
    b = (None, None) if bs is None else (bs[:, :3], bs[:, 3])
    if solver == capi.PCISPH:
        m = pcisph_model.run(p, x, va, *b, delta=stat, min_iters=iters, cap=iters)
        m["lam"], m["dx"] = m["p"], m["fp"]
    else:
        m = pbf_model.run(p, x, va, *b, eps=stat, min_iters=iters, eta=0.0, xsph=0.1)
    return dev, m


def _check(dev, m, tol=1e-4, what=""):
    assert dev["iters"] == m["iters"] == 3, what
    for nm, want in (("densCorr", m["rho"]), ("P_l", m["lam"]), ("forcesP", m["dx"]), ("posPred", m["xs"])):
        got = dev[nm][:, :3] if want.ndim == 2 else dev[nm]
        assert rel_err(got, want) <= tol, (what, nm, rel_err(got, want))
    assert rel_err(dev["pos"][:, :3], m["pos"]) <= tol, what
    assert rel_err(dev["vel"][:, :3], m["vel"]) <= 10 * tol, (what, rel_err(dev["vel"][:, :3], m["vel"]))
    assert rel_err(dev["pressure"], m["lam"]) <= tol, what


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("ref", [False, True])
def test_empty_and_one_particle(hip_lib, solver, ref):
    p, pos, vel = compressed_block()
    s = capi.Solver(p, 16, solver=solver, reference_order=ref)
    s.step(2)                       # empty: a no-op
    assert s.n == 0
    s.close()
    one = np.array([[0.1, 0.2, 0.3, 1.0]], np.float32)
    dev, m = _device_and_model(p, one, np.zeros_like(one), None, None, solver, ref)
    _check(dev, m, what="one")
    assert m["lam"][0] == 0 and dev["P_l"][0] == 0   # the self term alone is below rest density


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("ref", [False, True])
def test_ragged_sizes_and_walls(hip_lib, solver, ref):
    """63/64/65 and 255/256/257 particles of the 0.76 h compressed block (the solve has something to correct), and the small dam break
    squeezed to 0.87 with its walls"""
    p, pos, vel = compressed_block(ratio=0.76)
    for n in (63, 64, 65, 255, 256, 257):
        dev, m = _device_and_model(p, pos[:n], vel[:n], None, None, solver, ref)
        assert m["lam"].min() < 0 if solver == capi.PBF else m["lam"].max() > 0, n
        _check(dev, m, what=n)
    p2, sc = small_dam_break()
    dpos = sc["pos"].copy()
    lo = dpos[:, :3].min(axis=0)
    dpos[:, :3] = (lo + (dpos[:, :3] - lo) * 0.87).astype(dpos.dtype)
    dev, m = _device_and_model(p2, dpos, sc["vel"], sc["bi"], sc["vbi"], solver, ref)
    _check(dev, m, what="walls")


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("ref", [False, True])
def test_append_between_steps_equals_fresh_context(hip_lib, solver, ref):
    """Two steps of the 0.76 h block, then 10 particles appended (set_particles(..., first=s.n)): the next step equals a fresh context
    loaded with the concatenated state, bit for bit."""
    p, pos, vel = compressed_block(ratio=0.76)
    rng = np.random.default_rng(3)
    h = float(p["interactionRadius"][0])
    extra = np.ones((10, 4), np.float32)
    extra[:, :3] = (pos[:10, :3] + rng.uniform(-0.3 * h, 0.3 * h, (10, 3))).astype(np.float32)
    s = capi.Solver(p, len(pos) + 64, solver=solver, reference_order=ref)
    s.set_particles(pos, vel)
    s.step(2)
    xp, xv = s.download()
    s.set_particles(extra, None, first=s.n)
    assert s.n == len(pos) + 10
    s.step(1)
    got = list(s.download(pressure=True)) + [s.last_iterations]
    s.close()
    f = _solver(p, np.concatenate([xp, extra]), np.concatenate([xv, np.zeros_like(extra)]), solver=solver, reference_order=ref)
    f.step(1)
    want = list(f.download(pressure=True)) + [f.last_iterations]
    f.close()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
