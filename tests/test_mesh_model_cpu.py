"""The inputs of the mesh-sampling tests are not vacuous and stay clear of the undecided band: on the four cases of
tests/mesh_model.py (spacing 0.02) the numpy model finds the node counts below, the winding number of every node of a closed mesh is
an integer to within 3e-15, no node lies on the surface, and NO NODE HAS |w - 0.5| < 1e-6 — the condition under which the device's
selection (whose atan2 may differ from the host's in the last bits) must equal the model's node for node.  That is a condition on the
inputs, not a tolerance.  Also: the model-side mirrors of the kernel's constants, and the generators' triangle counts and orientation.
"""
import numpy as np
import pytest

from tests import mesh_model as mm

S = mm.S
# case -> (inside, shell <= s/2 inside, shell <= s/2 outside, fill with clearance s)
COUNTS = {"cube": (720, 216, 270, 336), "icosphere": (670, 164, 220, 358), "torus": (531, 240, 276, 139)}
MIN_DISTANCE = {"cube": 1.0e-3, "icosphere": 1.2e-5, "torus": 2.4e-5}  # smallest node-to-surface distance, to two digits


def test_constants_mirror_the_headers():
    assert mm.header_constant("nrs_kernels_mesh.h", "MESH_UNROLL") == mm.UNROLL
    assert mm.header_constant("nrs_host_mesh.h", "MESH_BATCH") == mm.BATCH == 1 << 22


def test_generators():
    assert len(mm.cube(mm.CUBE_LO, mm.CUBE_HI)[1]) == 12
    assert len(mm.icosphere(2)[1]) == 320 and len(mm.icosphere(2)[0]) == 162
    assert len(mm.torus(0.12, 0.045, 16, 8)[1]) == 2 * 16 * 8
    v, t = mm.cup(mm.CUBE_LO, mm.CUBE_HI)
    assert len(t) == 10
    # the cup is the cube without the two triangles of its +z face
    cv, ct = mm.cube(mm.CUBE_LO, mm.CUBE_HI)
    assert (ct[:10] == t).all() and (cv[ct[10:].astype(np.int64)][:, :, 2] == mm.CUBE_HI[2]).all()
    assert not (cv[ct[:10].astype(np.int64)][:, :, 2] == mm.CUBE_HI[2]).all(axis=1).any()
    for name in ("cube", "icosphere", "torus"):
        v, t = mm.case(name)[:2]
        # closed: every directed edge is matched by its reverse exactly once
        e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]).astype(np.int64)
        fwd = set(map(tuple, e.tolist()))
        assert len(fwd) == len(e) and fwd == set((b, a) for a, b in fwd)
        # wound counter-clockwise seen from outside: the signed volume is positive
        a, b, c = v[t[:, 0].astype(np.int64)], v[t[:, 1].astype(np.int64)], v[t[:, 2].astype(np.int64)]
        assert (a * np.cross(b, c)).sum() / 6.0 > 0.0


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_closed_cases(name):
    v, t, o, s, d = mm.case(name)
    assert s == S
    f = mm.case_field(name)
    w = f["winding"]
    inside, shell_in, shell_out, fill = COUNTS[name]
    assert int((w > 0.5).sum()) == inside
    shell = mm.selected(f, mm.INSIDE | mm.OUTSIDE, 0.0, S / 2)
    assert (int((shell & (w > 0.5)).sum()), int((shell & (w <= 0.5)).sum())) == (shell_in, shell_out)
    assert int(mm.selected(f, mm.INSIDE, S, np.inf).sum()) == fill
    assert np.abs(w - np.round(w)).max() < 3e-15
    dmin = float(np.sqrt(f["dist2"].min()))
    assert abs(dmin - MIN_DISTANCE[name]) <= 0.05 * MIN_DISTANCE[name] and dmin > 0.0
    assert (f["nearest"] < len(t)).all() and np.isfinite(f["closest"]).all()
    # the closest point is at the distance reported, bit for bit, and on the triangle's plane side of things: inside its bounding box
    P = mm.nodes(o, s, d)
    r = P - f["closest"]
    assert (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]).tobytes() == f["dist2"].tobytes()
    tri = v[t[f["nearest"].astype(np.int64)].astype(np.int64)]
    assert (f["closest"] >= tri.min(axis=1) - 1e-12).all() and (f["closest"] <= tri.max(axis=1) + 1e-12).all()


def test_cup():
    f = mm.case_field("cup")
    w = f["winding"]
    assert int((w > 0.5).sum()) == 720
    assert abs(np.abs(w - 0.5).min() - 5.1e-3) < 0.05e-3
    assert np.abs(w - np.round(w)).max() > 0.4  # open: the winding number is a genuine fraction somewhere


@pytest.mark.parametrize("name", mm.CASES)
def test_no_node_in_the_undecided_band(name):
    assert np.abs(mm.case_field(name)["winding"] - 0.5).min() >= 1e-6


def test_selections_are_not_vacuous():
    for name in mm.CASES:
        f = mm.case_field(name)
        n = len(f["dist2"])
        for flags, dmin, dmax in ((mm.INSIDE, S, np.inf), (mm.INSIDE | mm.OUTSIDE, 0.0, S / 2), (mm.OUTSIDE, 0.0, S / 2)):
            assert 0 < int(mm.selected(f, flags, dmin, dmax).sum()) < n


def test_model_ignores_batching_and_subsets():
    v, t, o, s, d = mm.case("torus")
    f = mm.case_field("torus")
    part = mm.field(v, t, mm.nodes(o, s, d, first=777, count=300))
    for k in part:
        assert part[k].tobytes() == f[k][777:1077].tobytes()
    only = mm.lattice_field(v, t, o, s, d, winding=False)
    assert sorted(only) == ["closest", "dist2", "nearest"] and only["dist2"].tobytes() == f["dist2"].tobytes()
