"""What every solver's context answers to every array id and every statistic, against a recording (tests/golden/solver_catalogue.json,
written by tests/golden/make_solver_catalogue.py on the MI355X from the commit before the routing of nrs_device_ptr and nrs_get_stat
moved into nrs_host_solver.h).  The refusal tests sample a handful of (solver, id) pairs; this one asks all of them: the five solvers
in fp32 Müller on small_dam_break (1,080 particles, the five-face box), PBF with the tensile correction and vorticity confinement on,
PCISPH and DFSPH with Akinci surface tension, and DFSPH once more with the divergence solve off.  At three moments per context —
after the upload, after step_partial(DENSITY), after one full step — every array id 0 .. 36 and every statistic 0 .. 12 is asked
twice by raw id: return code, message, byte count, the statistic's value as a hex float, and which ids share a device address.  Both
askings must agree (an answer changes nothing), and the recording holds one.  Every query is one the ABI answers with a code."""
import ctypes as C
import json
import os

import pytest

from nereus_amd import capi
from tests.common import small_dam_break

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_catalogue.json")
CASES = {"sesph": capi.SESPH, "iisph": capi.IISPH, "pcisph": capi.PCISPH, "pbf": capi.PBF, "dfsph": capi.DFSPH, "dfsph-nodiv": capi.DFSPH}
# the settings the recording was made with (as tests/test_dfsph_gpu.py's FIXED and tests/test_pbf_extras_gpu.py's K, DQ, EPS_V were then;
# written out here so that the recording depends on this file alone)
FIXED = (0.0, 3, 0.0, 3, 1)      # nrs_dfsph_configure: 3 + 3 iterations, warm start on, nothing read back
K, DQ, EPS_V = 1e-3, 0.3, 0.5    # PBF tensile k and dq, vorticity eps_v
ARRAY_IDS = range(0, 37)
STAT_IDS = range(0, 13)
# (case, moment, statistic id) whose code is compared and whose value is not: before the first step the four hit statistics are
# answered from hit counts no launch has written yet, whatever the allocation holds
UNSTABLE_VALUES = tuple((case, "fresh", which) for case in sorted(CASES) for which in (1, 2, 3, 4))


def _configure(s, case):
    """fixed iteration counts (no exit test reads anything back), every optional term of the solver on"""
    if case == "iisph":
        s.set_max_iterations(4)
    if case == "pcisph":
        s.pcisph_configure(0.01, 3)
        s.set_max_iterations(3)
        s.surface_akinci(1.0, 1.0)
    if case == "pbf":
        s.pbf_configure(0.0, 3, 0.01, 0.1)
        s.pbf_set_tensile(K, DQ)
        s.pbf_set_vorticity(EPS_V)
    if case == "dfsph":
        s.dfsph_configure(*FIXED)
        s.surface_akinci(1.0, 1.0)
    if case == "dfsph-nodiv":
        s.dfsph_configure(0.0, 3, 0.0, 0, 1)
        s.surface_akinci(1.0, 1.0)


def _message(lib, rc):
    return lib.nrs_last_error().decode() if rc else ""


def _moment(s):
    """every array id and every statistic, each asked twice with the same answer"""
    lib = s.lib
    where = []
    arrays, addr = {}, {}
    for which in ARRAY_IDS:
        asked = []
        for _ in range(2):
            p, b = C.c_void_p(), C.c_uint64()
            rc = lib.nrs_device_ptr(s.h, which, C.byref(p), C.byref(b))
            asked.append({"rc": rc, "msg": _message(lib, rc), "bytes": b.value if rc == 0 else None, "null": (not p.value) if rc == 0 else None})
            where.append(p.value if rc == 0 else None)
            if rc == 0 and p.value:
                addr.setdefault(p.value, set()).add(which)
        assert asked[0] == asked[1] and where[-1] == where[-2], ("array", which, asked)
        arrays[str(which)] = asked[0]
    stats = {}
    for which in STAT_IDS:
        asked = []
        for _ in range(2):
            v = C.c_double()
            rc = lib.nrs_get_stat(s.h, which, C.byref(v))
            asked.append({"rc": rc, "msg": _message(lib, rc), "value": float(v.value).hex() if rc == 0 else None})
        assert asked[0] == asked[1], ("statistic", which, asked)
        stats[str(which)] = asked[0]
    aliases = sorted(sorted(g) for g in addr.values() if len(g) > 1)
    return {"arrays": arrays, "stats": stats, "aliases": aliases}


def catalogue(case):
    """{"fresh" | "density" | "step": the answers at that moment, "calls": the codes of the steps between them} of one case"""
    p, sc = small_dam_break()
    s = capi.Solver(p, len(sc["pos"]), solver=CASES[case])
    lib = s.lib
    try:
        s.set_particles(sc["pos"], sc["vel"])
        s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
        _configure(s, case)
        out = {"fresh": _moment(s)}
        rc = lib.nrs_step_partial(s.h, capi.STAGE_DENSITY)
        calls = [{"rc": rc, "msg": _message(lib, rc)}]
        out["density"] = _moment(s)
        s.set_particles(sc["pos"], sc["vel"])   # (a partial step leaves the state mid-update)
        rc = lib.nrs_step(s.h, 1)
        calls.append({"rc": rc, "msg": _message(lib, rc)})
        s.synchronize()
        out["step"] = _moment(s)
        out["calls"] = calls
    finally:
        s.close()
    return out


def strip_unstable(rec, case):
    """a copy of one case's answers without the values listed in UNSTABLE_VALUES as (case, moment, statistic id)"""
    rec = json.loads(json.dumps(rec))
    for c, moment, which in UNSTABLE_VALUES:
        if c == case:
            rec[moment]["stats"][str(which)]["value"] = None
    return rec


@pytest.mark.parametrize("case", sorted(CASES))
def test_catalogue_equals_recording(hip_lib, case):
    with open(FIXTURE) as f:
        want = json.load(f)[case]
    got = strip_unstable(catalogue(case), case)
    assert sorted(got) == sorted(want)
    assert got["calls"] == want["calls"]
    for moment in ("fresh", "density", "step"):
        assert got[moment]["aliases"] == want[moment]["aliases"], (case, moment)
        for kind in ("arrays", "stats"):
            differ = [k for k in sorted(want[moment][kind], key=int) if got[moment][kind][k] != want[moment][kind][k]]
            assert not differ, "%s %s %s: ids %s differ from the recording, first: got %s want %s" % (
                case, moment, kind, differ, got[moment][kind][differ[0]], want[moment][kind][differ[0]])
