"""The implicit viscosity solve through the host class: Nereus::DFSPH::setImplicitViscosity forwards to nrs_dfsph_set_viscosity, and
`nereus_headless viscous <nu> <nu_b> <steps> <out.bin>` — the class on the shipped dam break — writes a finite state whose positions,
velocities and K equal those of the same steps through the C ABI, bit for bit."""
import subprocess

import numpy as np
import pytest

from nereus_amd import capi
from tests.common import default_scene
from tests.oracle_lib import SESPH
from tests.test_host_class import _driver, _read_out

pytestmark = pytest.mark.gpu


def _abi(got, pos, vel, steps, visc):
    s = capi.Solver(got["params"], len(pos), solver=capi.DFSPH)
    s.set_particles(pos, vel)
    s.set_boundaries(got["bi"], got["vbi"], update_grid=True)
    if visc is not None:
        s.dfsph_set_viscosity(*visc)
    for _ in range(steps):
        s.step(1)
    out = s.download(pressure=True), s.last_iterations, (s.dfsph_viscosity_info() if visc is not None else None)
    s.close()
    return out


@pytest.mark.parametrize("nu,nu_b", [(1.0, 0.0), (0.5, 0.25)])
def test_headless_viscous_equals_the_abi(tmp_path, hip_lib, nu, nu_b):
    steps = 4
    fout = str(tmp_path / "out.bin")
    text = subprocess.run([_driver(), "viscous", repr(nu), repr(nu_b), str(steps), fout], check=True, capture_output=True, text=True).stdout
    got = _read_out(fout)
    p, pos, vel = default_scene(SESPH)
    assert got["n"] == len(pos) and got["nb"] > 100000
    assert np.isfinite(got["pos"]).all() and np.isfinite(got["vel"]).all()
    (gp, gv, gk), iters, info = _abi(got, pos, vel, steps, (nu, nu_b, 1e-3, 1, 0))
    assert got["pos"].tobytes() == gp.tobytes()
    assert got["vel"].tobytes() == gv.tobytes()
    assert got["pressure"].tobytes() == gk.tobytes()
    assert got["iters"] == iters > 0
    assert info["on"] and ("viscous: on, %d CG iterations" % info["iterations"]) in text
    # the solve did something: the same steps without it end elsewhere
    (np_, _, _), _, _ = _abi(got, pos, vel, steps, None)
    assert got["pos"].tobytes() != np_.tobytes()
