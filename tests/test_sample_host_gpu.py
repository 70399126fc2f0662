"""Field sampling through the C++ host classes (Nereus::SPH::sampleLattice / getSampledDensity in nereus_amd/host) driven by the headless
driver's `lattice` mode: the file it writes equals nrs_sample_result of a ctypes run of the same scene and steps, bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

from nereus_amd import capi
from tests.common import small_dam_break
from tests.test_host_class import _driver, _write_in

pytestmark = pytest.mark.gpu
DIMS = (13, 9, 7)


def _lattice_run(tmp_path, kind, steps):
    p, sc = small_dam_break((12, 10, 9))
    h = float(p["interactionRadius"][0])
    origin = [float(v) for v in (sc["pos"][:, :3].astype(np.float64).min(0) - h)]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.lat")
    _write_in(fin, sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
    subprocess.check_call([_driver(), "lattice", kind, fin, str(steps)] + [repr(v) for v in origin] + [repr(h / 2)] + [str(d) for d in DIMS] + [fout],
                          stdout=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    assert struct.unpack_from("<4I", raw, 0) == DIMS + (32,)
    rho = np.frombuffer(raw, np.float32, offset=16)
    assert rho.size == DIMS[0] * DIMS[1] * DIMS[2] and len(raw) == 16 + 4 * rho.size
    return p, sc, h, origin, rho


def test_headless_lattice_equals_the_c_abi(tmp_path, hip_lib):
    steps = 4
    p, sc, h, origin, rho = _lattice_run(tmp_path, "sesph", steps)
    s = capi.Solver(p, len(sc["pos"]), solver=capi.SESPH)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    for _ in range(steps):   # (the host class sets the parameters and steps once per update())
        s.step(1)
    s.sample_lattice(origin, h / 2, DIMS, capi.FIELD_DENSITY)
    want = s.sample_result(capi.FIELD_DENSITY)
    assert want.max() > 0 and (want == 0).any()
    assert rho.tobytes() == want.tobytes()
    s.close()


def test_sample_lattice_through_the_pbf_class(tmp_path, hip_lib):
    """Nereus::PBF inherits the sampler from Nereus::SPH: it runs, and sees the fluid where the fluid is."""
    _, sc, h, origin, rho = _lattice_run(tmp_path, "pbf", 2)
    assert np.isfinite(rho).all() and rho.max() > 100.0 and (rho == 0).any()
    nodes = rho.reshape(DIMS[2], DIMS[1], DIMS[0])
    assert nodes[DIMS[2] // 2, DIMS[1] // 2, DIMS[0] // 2] > 0 and nodes[0, 0, 0] == 0  # a node inside the block, the corner a cell outside it
