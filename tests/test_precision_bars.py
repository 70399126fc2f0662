"""The fp64 parity bars (tests/test_parity_gpu.py TOL_STAGE_F64 / TOL_STEPS_F64) tell an fp64 build from an fp32 one: on the same
inputs the fp32 and fp64 oracles differ by at least 100x each bar.  CPU only (oracle against oracle)."""
import numpy as np
import pytest

from tests.common import compressed_block, rel_err, small_dam_break
from tests.oracle_lib import IISPH, SESPH, STOP_FORCES, STOP_I_PFORCE, Oracle
from tests.test_parity_gpu import TOL_STAGE_F64, TOL_STEPS_F64


def _pair(solver, kset, pos, vel, bi=None, vbi=None):
    out = []
    for double in (False, True):
        real = np.float64 if double else np.float32
        o = Oracle(Oracle.default_params(solver, double, kset), double, kset, solver, tait="double7", self_by_slot=kset == 0)
        o.set_particles(pos.astype(real), vel.astype(real))
        o.set_boundaries(None if bi is None else bi.astype(real), None if vbi is None else vbi.astype(real))
        out.append(o)
    return out


@pytest.mark.parametrize("kset", [1, 0], ids=["muller", "monaghan"])
def test_fp64_bars_separate_fp32_from_fp64_sesph(kset):
    """SESPH dam-break with walls (the fp32 scene, its inputs widened exactly): density, forces, 10-step positions."""
    p, sc = small_dam_break(kernel_set=kset)
    o32, o64 = _pair(SESPH, kset, sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
    for o in (o32, o64):
        o.step(1, stop=STOP_FORCES)
    np.testing.assert_array_equal(o32.get("index"), o64.get("index"))
    d = {"dens": rel_err(o32.get("dens"), o64.get("dens")), "forces": rel_err(o32.get("forces"), o64.get("forces"))}
    for o in (o32, o64):
        o.set_particles(sc["pos"].astype(o.real), sc["vel"].astype(o.real))
        o.step(10)
    d["pos10"] = rel_err(o32.get("pos")[:, :3], o64.get("pos")[:, :3])
    print(d)
    assert d["dens"] >= 100 * TOL_STAGE_F64 and d["forces"] >= 100 * TOL_STAGE_F64, d
    assert d["pos10"] >= 100 * TOL_STEPS_F64, d


@pytest.mark.parametrize("kset", [1, 0], ids=["muller", "monaghan"])
def test_fp64_bars_separate_fp32_from_fp64_iisph(kset):
    """IISPH on the compressed block of the new IISPH parity tests (Monaghan: spacing 0.58 h, self-exclusion by slot): every
    intermediate the fp64 stage bar is applied to, and the 5-step positions."""
    p, pos, vel = compressed_block(kernel_set=kset, ratio=0.72 if kset else 0.58)
    o32, o64 = _pair(IISPH, kset, pos, vel)
    for o in (o32, o64):
        o.step(1, stop=STOP_I_PFORCE)
    d = {nm: rel_err(o32.get(nm), o64.get(nm)) for nm in ("dens", "velAdv", "forcesAdv", "diiFluid", "densAdv", "aii", "sumDij",
                                                          "densCorr", "P_l", "pres", "forcesP")}
    for o in (o32, o64):
        o.set_particles(pos.astype(o.real), vel.astype(o.real))
        o.step(5)
    d["pos5"] = rel_err(o32.get("pos")[:, :3], o64.get("pos")[:, :3])
    print(d)
    for nm, e in d.items():
        assert e >= 100 * (TOL_STEPS_F64 if nm == "pos5" else TOL_STAGE_F64), (nm, d)
