"""NRS_FLAG_STAGED_SCAN and NRS_FLAG_STAGED_SCAN | NRS_FLAG_FAST_ARITH (k_density_staged, nrs_kernels_staged.h) on small scenes built
to enter its data-dependent branches: tail waves, the edge-cell and pool fall-backs to the global-memory scan, hulls of 65-128 and
of more than 128 candidates, list overflow inside staged waves, both wall sweeps, and a boundary cell beyond the 11-bit offsets of
the FAST lists.  tests/test_staged_model_cpu.py shows on the numpy model (tests/staged_model.py) that each scene contains its
branch; here the exact launch equals the reference-order context bit for bit (and the CPU oracle's density), the FAST launch is
within the mode's bar of the oracle, and the launch's statistics equal the model's.  No expected value comes from the device."""
import numpy as np
import pytest

from nereus_amd import capi
from tests import staged_model as sm
from tests.common import check_cell_tables, close_masked

pytestmark = pytest.mark.gpu

TOL = 1e-5   # the FAST mode's bar, array-relative (tests/test_fast_arith_gpu.py)
SCENES = sm.targeted_scenes()
_reference = {}


def _solver(s, **kw):
    d = capi.Solver(s["p"], max(len(s["pos"]), 1), **kw)
    d.set_particles(s["pos"], s["vel"])
    d.set_boundaries(s["bi"], s["vbi"], update_grid=False)
    return d


def _reference_order(name):
    """the reference-order context's partial steps of a scene, once"""
    if name not in _reference:
        d = _solver(SCENES[name], reference_order=True)
        d.step_partial(capi.STAGE_DENSITY)
        out = {"density " + k: d.get(k) for k in ("dens", "pres")}
        d.set_particles(SCENES[name]["pos"], SCENES[name]["vel"])
        d.step_partial(capi.STAGE_FORCES)
        out.update({k: d.get(k) for k in ("hash", "index", "cellStart", "cellEnd", "dens", "pres", "forces")})
        d.close()
        _reference[name] = out
    return _reference[name]


def _indices_equal_oracle(d, st):
    np.testing.assert_array_equal(d.get("hash"), st["hash"])
    np.testing.assert_array_equal(d.get("index"), st["index"])
    check_cell_tables(d.get("cellStart"), d.get("cellEnd"), st["cellStart"], st["cellEnd"])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_staged_scan_exact(hip_lib, name):
    s, st, m, ref = SCENES[name], sm.oracle_state(name, SCENES[name]), sm.predict_scene(name, SCENES[name]), _reference_order(name)
    d = _solver(s, flags=capi.FLAG_STAGED_SCAN)
    d.step_partial(capi.STAGE_DENSITY)   # the launches without shared lists
    for k in ("dens", "pres"):
        np.testing.assert_array_equal(d.get(k), ref["density " + k], err_msg="STAGE_DENSITY " + k)
    d.set_particles(s["pos"], s["vel"])
    d.step_partial(capi.STAGE_FORCES)
    _indices_equal_oracle(d, st)
    for k in ("dens", "pres", "forces"):
        np.testing.assert_array_equal(d.get(k), ref[k], err_msg=k)
    np.testing.assert_array_equal(d.get("dens"), st["dens"])
    d.set_particles(s["pos"], s["vel"])
    d.step(1)   # (the statistics are those of a completed step: its density launch ran on the same uploaded state)
    got = {k: int(d.get_stat(v)) for k, v in (("stat_unstaged", capi.STAT_UNSTAGED), ("stat_hit_overflow", capi.STAT_HIT_OVERFLOW),
                                              ("stat_hit_max", capi.STAT_HIT_MAX))}
    d.close()
    assert got == {k: m[k] for k in got}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_staged_scan_fast(hip_lib, name):
    s, st, m = SCENES[name], sm.oracle_state(name, SCENES[name]), sm.predict_scene(name, SCENES[name])
    d = _solver(s, flags=capi.FLAG_STAGED_SCAN | capi.FLAG_FAST_ARITH)
    d.step_partial(capi.STAGE_DENSITY)   # (without shared lists the plan keeps the exact arithmetic: the bar holds all the more)
    close_masked(d.get("dens"), st["dens"], TOL, name + " STAGE_DENSITY dens")
    d.set_particles(s["pos"], s["vel"])
    d.step_partial(capi.STAGE_FORCES)
    _indices_equal_oracle(d, st)
    dens, forces = d.get("dens"), d.get("forces")
    d.set_particles(s["pos"], s["vel"])
    d.step(1)   # (the statistics are those of a completed step)
    unstaged, over = int(d.get_stat(capi.STAT_UNSTAGED)), int(d.get_stat(capi.STAT_HIT_OVERFLOW))
    d.close()
    close_masked(dens, st["dens"], TOL, name + " dens")
    close_masked(forces, st["forces"], TOL, name + " forces")
    assert unstaged == m["stat_unstaged"]
    # (a boundary cell of more than 2048 particles overflows lists the exact launch keeps: never fewer than the model's)
    assert over >= m["stat_hit_overflow"] if name.startswith("b2100") else over == m["stat_hit_overflow"]
