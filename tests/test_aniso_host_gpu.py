"""The anisotropic surface reconstruction through the C++ host classes (Nereus::SPH::extractSurfaceAniso in nereus_amd/host) driven by
the headless driver's `surface ... --aniso [support]` mode: the Wavefront OBJ it writes has the vertices (read back bit for bit) and the
1-based triangle indices of nrs_surface_result after nrs_surface_extract_aniso in a ctypes run of the same scene and steps; and
Nereus::DFSPH inherits the methods."""
import subprocess

import numpy as np
import pytest

from nereus_amd import capi
from tests import aniso_model as am
from tests import surface_model as sm
from tests.common import small_dam_break
from tests.test_host_class import _driver, _write_in

pytestmark = pytest.mark.gpu


def _obj_run(tmp_path, kind, steps, sc, origin, spacing, dims, iso, *aniso):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.obj")
    _write_in(fin, sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
    subprocess.check_call([_driver(), "surface", kind, fin, str(steps)] + [repr(v) for v in origin] + [repr(spacing)] + [str(d) for d in dims] +
                          [repr(iso), fout] + list(aniso), stdout=subprocess.DEVNULL)
    v, f = [], []
    for line in open(fout):
        w = line.split()
        if w and w[0] == "v":
            v.append([float(x) for x in w[1:]])
        elif w and w[0] == "f":
            f.append([int(x) for x in w[1:]])
        else:
            assert not w or w[0] == "#", line
    return np.array(v, np.float64).reshape(-1, 3), np.array(f, np.int64).reshape(-1, 3)


@pytest.mark.parametrize("support", [None, 1.25], ids=["default", "support-1.25h"])
def test_headless_aniso_surface_equals_the_c_abi(tmp_path, hip_lib, support):
    steps = 3
    p, sc = small_dam_break((12, 10, 9))
    h = float(p["interactionRadius"][0])
    origin, dims = am.padded_lattice(sc["pos"], h, h / 2, 2.5)
    extra = ["--aniso"] + ([repr(support * h)] if support else [])
    v, f = _obj_run(tmp_path, "sesph", steps, sc, origin, h / 2, dims, 0.5, *extra)
    s = capi.Solver(p, len(sc["pos"]), solver=capi.SESPH)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    for _ in range(steps):   # (the host class sets the parameters and steps once per update())
        s.step(1)
    V, T = s.surface_extract_aniso(origin, h / 2, dims, 0.5, 0, dict(support=support * h) if support else None)
    want_v, want_t = s.surface_result(capi.MESH_VERTICES), s.surface_result(capi.MESH_TRIANGLES)
    assert V > 200 and (len(v), len(f)) == (V, T)
    assert v.astype(np.float32).tobytes() == np.ascontiguousarray(want_v[:, :3]).tobytes()
    assert np.array_equal(f - 1, want_t.astype(np.int64))
    sm.mesh_checks(v, f - 1, closed=True)
    # not the density's surface: that call on the same state gives another mesh
    assert s.surface_extract(origin, h / 2, dims, 0.5 * float(p["restDensity"][0]), 0) != (V, T)
    s.close()


def test_aniso_surface_through_the_dfsph_class(tmp_path, hip_lib):
    """Nereus::DFSPH inherits the methods from Nereus::SPH: one closed, outward-wound surface around the fluid"""
    p, sc = small_dam_break((12, 10, 9))
    h = float(p["interactionRadius"][0])
    origin, dims = am.padded_lattice(sc["pos"], h, h / 2, 2.5)
    v, f = _obj_run(tmp_path, "dfsph", 2, sc, origin, h / 2, dims, 0.5, "--aniso")
    assert len(v) > 200 and f.min() == 1 and f.max() == len(v)
    chi, vol = sm.mesh_checks(v, f - 1, closed=True)
    assert am.components(f - 1, len(v)) == 1 and chi == 2
    ext = sc["pos"][:, :3].astype(np.float64)
    box = float(np.prod(ext.max(0) - ext.min(0)))
    assert 0.9 * box < vol < 1.5 * box
