"""Mesh sampling through the C++ host side (sample_spheres::ss::sampleMesh, Nereus::SPH::emitMesh in nereus_amd/host) driven by the
headless driver's `mesh <in.obj> <spacing> <fill|shell> <out.bin>` mode: what it writes is, byte for byte, capi.mesh_particles on the
lattice and with the rules those two document; an OBJ with quads and a/b/c corners loads to the fanned triangles; and the OBJ the
driver's own surface mode writes loads and has an inside."""
import subprocess

import numpy as np
import pytest

from nereus_amd import capi
from tests import aniso_model as am
from tests import mesh_model as mm
from tests.common import small_dam_break
from tests.test_aniso_host_gpu import _obj_run
from tests.test_host_class import _driver

pytestmark = pytest.mark.gpu

S = mm.S


def mesh_lattice(v, radius):
    """ss::meshLattice: pitch radius, the bounding box plus one node on every side"""
    v = np.asarray(v, np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    return tuple(lo - radius), radius, tuple(int(x) for x in np.floor((hi - lo) / radius) + 3.0)


def rules(radius):
    return {"shell": (capi.MESH_INSIDE | capi.MESH_OUTSIDE | capi.MESH_SNAP, 0.0, radius / 2), "fill": (capi.MESH_INSIDE, radius / 2, np.inf)}


def headless_mesh(tmp_path, obj, spacing, what):
    fout = str(tmp_path / ("%s.bin" % what))
    subprocess.check_call([_driver(), "mesh", str(obj), repr(float(spacing)), what, fout], stdout=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    n, precision = (int(x) for x in np.frombuffer(raw[:8], np.uint32))
    assert precision == 32 and len(raw) == 8 + 16 * n
    return np.frombuffer(raw, np.float32, 4 * n, 8).reshape(-1, 4)


def want(v, t, spacing, what):
    o, s, d = mesh_lattice(v, spacing)
    flags, dmin, dmax = rules(spacing)[what]
    return capi.mesh_particles(v, t, o, s, d, flags=flags, dmin=dmin, dmax=dmax)


@pytest.mark.parametrize("what", ["fill", "shell"])
def test_headless_mesh_equals_the_c_abi(tmp_path, hip_lib, what):
    v, t = mm.case("icosphere")[:2]
    obj = tmp_path / "ico.obj"
    mm.write_obj(obj, v, t)
    got = headless_mesh(tmp_path, obj, S, what)
    ref = want(v, t, S, what)
    assert len(ref) > 100 and got.tobytes() == ref.tobytes()
    # and the model agrees (the lattice is not the case's own: its band is checked here)
    o, s, d = mesh_lattice(v, S)
    f = mm.lattice_field(v, t, o, s, d)
    assert np.abs(f["winding"] - 0.5).min() >= 1e-6
    assert got.tobytes() == mm.particles(f, mm.nodes(o, s, d), *rules(S)[what], np.float32).tobytes()


def test_obj_with_quads_and_slashes(tmp_path, hip_lib):
    v, t = mm.case("cube")[:2]
    quads = [(t[2 * k][0], t[2 * k][1], t[2 * k][2], t[2 * k + 1][2]) for k in range(6)]
    fanned = np.array([x for q in quads for x in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.uint32)
    assert (fanned == t).all()
    obj = tmp_path / "quads.obj"
    with open(obj, "w") as fh:
        fh.write("# a cube of six quads\no cube\nvn 0 0 1\nvt 0.5 0.5\n")
        for x in v:
            fh.write("v  %.17g %.17g\t%.17g\n" % tuple(x))
        for k, q in enumerate(quads):
            form = ("%d/1/1", "%d//1", "%d/1", "%d")[k % 4]
            corners = [(int(i) + 1) if k != 5 else int(i) - len(v) for i in q]  # the last face counts from the end
            fh.write("f " + " ".join(form % c for c in corners) + "\n")
    for what in ("fill", "shell"):
        got = headless_mesh(tmp_path, obj, S, what)
        assert len(got) > 50 and got.tobytes() == want(v, t, S, what).tobytes()


def test_surface_obj_round_trip(tmp_path, hip_lib):
    p, sc = small_dam_break((12, 10, 9))
    h = float(p["interactionRadius"][0])
    origin, dims = am.padded_lattice(sc["pos"], h, h / 2, 2.5)
    v, f = _obj_run(tmp_path, "sesph", 3, sc, origin, h / 2, dims, 0.5, "--aniso")
    assert len(sc["pos"]) == 1080 and len(v) > 200
    t = (f - 1).astype(np.uint32)
    nodes = int(dims[0]) * int(dims[1]) * int(dims[2])
    inside = capi.mesh_particles(v, t, origin, h / 2, dims, flags=capi.MESH_INSIDE, count_only=True)
    assert 0 < inside < nodes
    # the fluid's bounding box has about that many nodes of the extraction lattice
    ext = sc["pos"][:, :3].astype(np.float64)
    box = float(np.prod((ext.max(0) - ext.min(0)) / (h / 2)))
    assert 0.8 * box < inside < 1.7 * box
    # the driver reads its own output
    got = headless_mesh(tmp_path, tmp_path / "out.obj", h / 2, "fill")
    assert len(got) > 100 and got.tobytes() == want(v, t, h / 2, "fill").tobytes()
