"""Diffuse particles through the C++ host classes (Nereus::SPH::configureDiffuse / stepDiffuse / getDiffuse in nereus_amd/host) driven
by the headless driver's `diffuse` mode: the living set it writes is, byte for byte, that of nrs_diffuse_result in a ctypes run of the
same scene, steps and configuration."""
import subprocess

import numpy as np
import pytest

from nereus_amd import capi
from tests.common import small_dam_break
from tests.test_host_class import _driver, _write_in

pytestmark = pytest.mark.gpu

# the configuration of `nereus_headless diffuse` (host/tools/headless.cpp)
HEADLESS = dict(capacity=1 << 20, seed=0, tau_ta=(0.1, 0.5), tau_wc=(0.1, 1.0), tau_k=(5e-4, 4e-3), k_ta=3000.0, k_wc=3000.0, lifetime=(0.5, 2.0),
                k_buoyancy=2.0, k_drag=0.8, spray_below=6, bubble_above=20, max_per_particle=3)


def test_headless_diffuse_equals_the_c_abi(tmp_path, hip_lib):
    steps = 4
    p, sc = small_dam_break((12, 10, 9))
    vel = sc["vel"].copy()
    vel[:, :3] = np.random.default_rng(11).uniform(-0.3, 0.3, (len(vel), 3))
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.dif")
    _write_in(fin, sc["pos"], vel, sc["bi"], sc["vbi"])
    subprocess.check_call([_driver(), "diffuse", "sesph", fin, str(steps), fout], stdout=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    count, precision = np.frombuffer(raw[:8], np.uint32)
    assert precision == 32 and len(raw) == 8 + count * (16 + 16 + 4)
    pos = np.frombuffer(raw, np.float32, 4 * count, 8).reshape(-1, 4)
    v = np.frombuffer(raw, np.float32, 4 * count, 8 + 16 * count).reshape(-1, 4)
    kind = np.frombuffer(raw, np.uint32, count, 8 + 32 * count)
    s = capi.Solver(p, len(sc["pos"]), solver=capi.SESPH)
    s.set_particles(sc["pos"], vel)
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    s.diffuse_configure(**HEADLESS)
    for _ in range(steps):   # (the host class sets the parameters and steps once per update())
        s.step(1)
        s.diffuse_step()
    assert s.diffuse_count()[0] == count and count > 100
    assert pos.tobytes() == s.diffuse_result(capi.DIFFUSE_POS).tobytes()
    assert v.tobytes() == s.diffuse_result(capi.DIFFUSE_VEL).tobytes()
    assert kind.tobytes() == s.diffuse_result(capi.DIFFUSE_KIND).tobytes()
    s.close()
