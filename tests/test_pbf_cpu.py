"""PBF without a GPU: the ABI declares the solver, the model's D_proto has the closed form of a six-neighbour prototype, and the model
converges on the compressed block that PCISPH does not."""
import os
import re

import numpy as np
import pytest

from nereus_amd import capi
from tests import pbf_model
from tests.common import compressed_block
from tests.oracle_lib import IISPH, SESPH, Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_pbf():
    text = open(os.path.join(ROOT, "include", "nereus_hip.h")).read()
    assert re.search(r"NRS_SOLVER_PBF\s*=\s*3\b", text)
    assert re.search(r"\bint\s+nrs_pbf_configure\s*\(\s*nrs_ctx\s*\*\s*\w+\s*,\s*double\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*double\s+\w+\s*,"
                     r"\s*double\s+\w+\s*\)", text)
    for name, value in (("NRS_STAT_PBF_EPSILON", 7), ("NRS_STAT_DENSITY_ERROR", 5), ("NRS_STAGE_P_ADVECT", 7), ("NRS_STAGE_P_SOLVE", 8),
                        ("NRS_STAGE_P_INTEGRATE", 9), ("NRS_STAGE_COUNT", 16)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text), name
    assert capi.PBF == 3
    assert capi.STAT_PBF_EPSILON == 7
    assert "nrs_pbf_configure" in capi.EXPORTS
    assert hasattr(capi.Solver, "pbf_configure")


@pytest.mark.parametrize("solver", [SESPH, IISPH])
@pytest.mark.parametrize("double", [False, True])
def test_model_d_proto_of_six_neighbour_prototype(solver, double):
    """On the lattice of spacing cbrt(m / rho0) = 0.794 h the prototype has six neighbours, sum g = 0, and D_proto = 6 (m / rho0)^2
    |grad W_spiky(s)|^2."""
    p = Oracle.default_params(solver, double)
    m, rd, h = (float(p[k][0]) for k in ("particleMass", "restDensity", "interactionRadius"))
    real = np.float64 if double else np.float32
    s = float(real(np.cbrt(m / rd)))
    d, count = pbf_model.prototype_d(p)
    assert count == 6
    g = pbf_model.spiky_grad(np.array([[s, 0.0, 0.0]]), h, float(p["kpress_grad"][0]))[0]
    want = 6.0 * (m / rd) ** 2 * float(g @ g)
    np.testing.assert_allclose(d, want, rtol=1e-6 if not double else 1e-12)
    if solver == IISPH:
        assert 190 < d < 197   # ~193 m^-2 with the IISPH constructor's parameters


def test_model_spiky_gradient_is_zero_at_zero_separation():
    p = Oracle.default_params(IISPH, True)
    h, kpg = float(p["interactionRadius"][0]), float(p["kpress_grad"][0])
    g = pbf_model.spiky_grad(np.array([[0.0, 0.0, 0.0], [0.1 * h, 0.0, 0.0], [1.5 * h, 0.0, 0.0]]), h, kpg)
    assert np.all(np.isfinite(g))
    assert np.all(g[0] == 0) and np.all(g[2] == 0) and g[1, 0] != 0


@pytest.mark.parametrize("double", [False, True])
def test_model_converges_on_compressed_block(double):
    """The 0.72 h block (34 % over rest density), start state at rest: max e <= 0.01 after 12 iterations (PCISPH diverges on it,
    DESIGN.md "PCISPH"), and 0 by iteration 50."""
    p, pos, vel = compressed_block(double=double)
    r = pbf_model.run(p, pos, np.zeros_like(pos), min_iters=1, eta=0.01)
    assert r["iters"] == 12, r["errors"]
    assert r["errors"][0] > 0.3 and r["errors"][-1] <= 0.01
    r = pbf_model.run(p, pos, np.zeros_like(pos), min_iters=50, eta=0.01)
    assert r["iters"] == 50 and r["errors"][-1] <= 1e-6
    f = pbf_model.run(p, pos, np.zeros_like(pos), min_iters=4, eta=0.0)   # fixed-count mode ignores eta and the cap
    assert f["iters"] == 4
    assert np.all(f["lam"] <= 0) and np.all(np.isfinite(f["xs"]))
