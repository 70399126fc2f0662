"""Sources and sinks through the C++ host classes (Nereus::SPH::setEmitter / setSinks / getEmitter / sinkCounts in nereus_amd/host) driven
by the headless driver's `faucet` mode: the final set and the counts it writes are, byte for byte, those of a ctypes run of the same
emitter, sink and steps."""
import subprocess

import numpy as np
import pytest

from nereus_amd import capi
from tests.oracle_lib import Oracle
from tests.test_host_class import _driver

pytestmark = pytest.mark.gpu

STEPS = 120


def test_headless_faucet_equals_the_c_abi(tmp_path, hip_lib):
    fout = str(tmp_path / "out.bin")
    subprocess.check_call([_driver(), "faucet", "sesph", str(STEPS), fout], stdout=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    n, precision = np.frombuffer(raw[:8], np.uint32)
    emitted, dropped, removed, culls = (int(x) for x in np.frombuffer(raw[8:40], np.uint64))
    assert precision == 32 and len(raw) == 40 + n * 32
    pos = np.frombuffer(raw, np.float32, 4 * n, 40).reshape(-1, 4)
    vel = np.frombuffer(raw, np.float32, 4 * n, 40 + 16 * n).reshape(-1, 4)
    p = Oracle.default_params(capi.SESPH, False, capi.MULLER)
    s = capi.Solver(p, 150000, solver=capi.SESPH)
    r = 2.5 * float(np.cbrt(np.float64(p["particleMass"][0]) / np.float64(p["restDensity"][0])))
    s.emitter_set(0, center=(0.0, -0.9, 0.0), direction=(0.0, -1.0, 0.0), half_extent=(r, 0.0), speed=4.0, shape=capi.EMITTER_DISC)
    s.sinks_set([], domain=True)
    for _ in range(STEPS):  # (the host class sets the parameters and steps once per update())
        s.step(1)
    assert (s.n, s.emitter_get(0)[1:], s.sinks_count()) == (n, (emitted, dropped), (removed, culls))
    assert emitted > 200 and removed > 0 and dropped == 0 and culls == STEPS and n == emitted - removed
    gp, gv = s.download()
    assert pos.tobytes() == gp.tobytes() and vel.tobytes() == gv.tobytes()
    s.close()
