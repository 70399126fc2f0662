"""The bits of the PCISPH, PBF, DFSPH and Akinci kernels against a recording (tests/golden/solver_bits.json, written by
tests/golden/make_solver_bits.py on the MI355X from the commit before the neighbour passes were given one shared walk).  The
list-versus-reference-order tests compare the two kernel paths with each other and would not see both drift together; this one pins
each of them: SHA-256 digests of every array those tests read back, at DENSITY, P_ADVECT and P_SOLVE (3 fixed iterations) and after
two full steps, on the four scenes of tests/test_pcisph_gpu.py's bitwise test (two of them overflow their hit lists) and, for DFSPH's
wall-velocity term, on the moving-plate scene of tests/test_bodies_gpu.py."""
import hashlib
import json
import os

import numpy as np
import pytest

from nereus_amd import capi
from tests import test_bodies_gpu as bodies
from tests.oracle_lib import Oracle
from tests.test_dfsph_gpu import FIXED, _moving
from tests.test_pbf_extras_gpu import DQ, EPS_V, K
from tests.test_pcisph_gpu import _bitwise_scenes

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_bits.json")
# (name, double, kernel set, reference-order kernels, flags); "nowalls": the list kernels with boundary code in every workgroup
BUILDS = [("f32-muller-lists", False, capi.MULLER, False, 0), ("f32-muller-ref", False, capi.MULLER, True, 0),
          ("f64-muller-lists", True, capi.MULLER, False, 0), ("f32-monaghan", False, capi.MONAGHAN, False, 0),
          ("f32-muller-lists-nowalls", False, capi.MULLER, False, capi.FLAG_NO_WALL_WORKGROUPS)]
SOLVERS = ["pcisph", "pbf", "dfsph", "akinci", "dfsph-bodies"]
CASES = ["%s/%s" % (b[0], s) for b in BUILDS for s in SOLVERS]
PCI_ADVECT = ["dens", "velAdv", "forcesAdv", "posPred"]
PCI_SOLVE = ["densCorr", "P_l", "forcesP", "posPred", "pres"]
# per solver: the arrays read back at DENSITY, P_ADVECT, P_SOLVE and, besides pos, vel and pressure, after the full steps
ARRAYS = {"pcisph": (["dens"], PCI_ADVECT, PCI_SOLVE, []),
          "pbf": (["dens"], PCI_ADVECT, PCI_SOLVE, ["vorticity"]),
          "dfsph": (["dens", "dfsphAlpha", "pres", "dfsphKappaV"], ["sortedVel", "velAdv", "forcesAdv", "dfsphKappaV"],
                    ["velAdv", "pres", "P_l", "densCorr"], ["dfsphKappaV", "dfsphAlpha"]),
          "akinci": (["dens"], ["normals"] + PCI_ADVECT, PCI_SOLVE, [])}
ARRAYS["dfsph-bodies"] = ARRAYS["dfsph"]
STAGES = (("density", capi.STAGE_DENSITY), ("p_advect", capi.STAGE_P_ADVECT), ("p_solve", capi.STAGE_P_SOLVE))


def _configure(s, solver):
    """3 fixed iterations of every solve, and every optional term of the solver on"""
    if solver in ("pcisph", "akinci"):
        s.pcisph_configure(0.01, 3)
        s.set_max_iterations(3)
    if solver == "akinci":
        s.surface_akinci(1.0, 1.0)
    if solver == "pbf":
        s.pbf_configure(0.0, 3, 0.01, 0.1)
        s.pbf_set_tensile(K, DQ)
        s.pbf_set_vorticity(EPS_V)
    if solver in ("dfsph", "dfsph-bodies"):
        s.dfsph_configure(*FIXED)


def _scenes(solver, double, kernel_set):
    """(make a configured context, (pos, vel) to start a stop from) per scene"""
    real = np.float64 if double else np.float32
    if solver == "dfsph-bodies":
        sc = bodies.scene(double, kernel_set, plate_gap=0.0457 - 0.005, squeeze=0.87)
        return [(lambda **kw: bodies.make(sc, capi.DFSPH, plate_v=(2.4, 0.0, 0.0), double=double, kernel_set=kernel_set, **kw),
                 sc[1], sc[2])]
    kind = {"pcisph": capi.PCISPH, "akinci": capi.PCISPH, "pbf": capi.PBF, "dfsph": capi.DFSPH}[solver]
    out = []
    for p, pos, vel, bi, vbi, _ in _bitwise_scenes():
        p = Oracle.recompute_constants(p, double, kernel_set)
        pos, vel = pos.astype(real), (_moving(vel) if solver == "dfsph" else vel).astype(real)
        bi, vbi = (None, None) if bi is None else (bi.astype(real), vbi.astype(real))

        def make(p=p, pos=pos, vel=vel, bi=bi, vbi=vbi, **kw):
            s = capi.Solver(p, len(pos), solver=kind, double=double, kernel_set=kernel_set, **kw)
            s.set_particles(pos, vel)
            s.set_boundaries(bi, vbi, update_grid=True)
            return s
        out.append((make, pos, vel))
    return out


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digests(case):
    """{"scene/stop/array": SHA-256 of the array's bytes} of one case, "build/solver".  A fresh context per stop: the moving bodies of
    the bodies scene start from their first pose at each, like the particles."""
    build, solver = case.split("/")
    _, double, kernel_set, ref, flags = next(b for b in BUILDS if b[0] == build)
    at_density, at_advect, at_solve, at_end = ARRAYS[solver]
    out = {}
    for k, (make, pos, vel) in enumerate(_scenes(solver, double, kernel_set)):
        for (stop, stage), names in zip(STAGES, (at_density, at_advect, at_solve)):
            s = make(reference_order=ref, flags=flags)
            _configure(s, solver)
            s.step_partial(stage)
            for nm in names:
                out["%d/%s/%s" % (k, stop, nm)] = _sha(s.get(nm))
            if stop == "p_solve":
                out["%d/%s/iterations" % (k, stop)] = int(s.last_iterations)
            s.close()
        s = make(reference_order=ref, flags=flags)
        _configure(s, solver)
        s.step(2)
        for nm, a in zip(("pos", "vel", "pressure"), s.download(pressure=True)):
            out["%d/steps/%s" % (k, nm)] = _sha(a)
        for nm in at_end:
            out["%d/steps/%s" % (k, nm)] = _sha(s.get(nm))
        out["%d/steps/iterations" % k] = int(s.last_iterations)
        s.close()
    return out


@pytest.mark.parametrize("case", CASES)
def test_bits_equal_recording(hip_lib, case):
    with open(FIXTURE) as f:
        want = json.load(f)[case]
    got = digests(case)
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, "%s: %d of %d differ from the recording: %s" % (case, len(differ), len(want), differ[:12])
