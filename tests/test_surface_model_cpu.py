"""The numpy model of the surface extraction (tests/surface_model.py) on analytic fields, without a GPU: the surface of a field that
is below iso on the lattice boundary is a closed, consistently oriented manifold in which every vertex is used, with the Euler
characteristic of the shape; a surface cut by the boundary keeps "every directed edge at most once"; and on a field that is concave
along every edge (c - r) every vertex lies inside the sphere, which bounds the enclosed volume from both sides.
"""
import numpy as np
import pytest

from tests import surface_model as sm

DIMS = (14, 14, 14)
ISO = 1.0


def nodes_xyz(origin, spacing, dims):
    ax = sm.lattice_axes(origin, spacing, dims, np.float64)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return x.ravel(), y.ravel(), z.ravel()


def sphere(c=(6.4, 6.6, 6.3), R=4.2):
    x, y, z = nodes_xyz((0, 0, 0), 1.0, DIMS)
    return ISO + (R - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2))


def two_blobs():
    """two balls on integer nodes with integer squared radii: the nodes with r^2 == R^2 have the density iso exactly"""
    x, y, z = nodes_xyz((0, 0, 0), 1.0, DIMS)
    a = ISO + (5.0 - ((x - 3) ** 2 + (y - 3) ** 2 + (z - 3) ** 2)) / 8.0
    b = ISO + (9.0 - ((x - 9) ** 2 + (y - 9) ** 2 + (z - 9) ** 2)) / 8.0
    return np.maximum(a, b)


def torus(c=6.5, major=4.0, minor=1.6):
    x, y, z = nodes_xyz((0, 0, 0), 1.0, DIMS)
    ring = np.sqrt((x - c) ** 2 + (y - c) ** 2) - major
    return ISO + (minor - np.sqrt(ring ** 2 + (z - c) ** 2))


@pytest.mark.parametrize("real", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("field,chi,at_iso", [(sphere, 2, 0), (two_blobs, 4, 54), (torus, 0, 0)], ids=["sphere", "two-blobs", "torus"])
def test_closed_surfaces(field, chi, at_iso, real):
    f = field().astype(real)
    assert int((f == real(ISO)).sum()) == at_iso
    m = sm.extract(f, (0, 0, 0), 1.0, DIMS, ISO, real)
    assert m["V"] > 100 and m["T"] > 200 and m["cell_counts"].sum() == m["T"] and m["cell_counts"].max() <= 12
    got_chi, vol = sm.mesh_checks(m["vertices"], m["triangles"], closed=True, lattice_volume=13.0 ** 3)
    assert got_chi == chi
    t = m["vertices"][:, 3]
    assert (t >= 0).all() and (t <= 1).all()
    if at_iso:
        assert (t == 0).sum() > 0  # an owner exactly at iso is inside: its crossing edges have t == 0 ...
        assert (t == 1).sum() > 0  # ... and a far end exactly at iso t == 1


def test_sphere_volume_is_bounded_from_both_sides():
    R = 4.2
    m = sm.extract(sphere(R=R), (0, 0, 0), 1.0, DIMS, ISO, np.float64)
    _, vol = sm.mesh_checks(m["vertices"], m["triangles"], closed=True)
    x = m["vertices"][:, :3] - np.array((6.4, 6.6, 6.3))
    r = np.sqrt((x ** 2).sum(1))
    assert (r <= R + 1e-12).all() and (r >= R - np.sqrt(3.0)).all()
    assert 4 / 3 * np.pi * (R - np.sqrt(3.0)) ** 3 < vol < 4 / 3 * np.pi * R ** 3


def test_cut_by_the_boundary_is_open_but_oriented():
    f = sphere(c=(1.2, 6.6, 6.3))
    m = sm.extract(f, (0, 0, 0), 1.0, DIMS, ISO, np.float64)
    assert m["T"] > 100
    sm.mesh_checks(m["vertices"], m["triangles"], closed=False)
    with pytest.raises(AssertionError):
        sm.mesh_checks(m["vertices"], m["triangles"], closed=True)


def test_anisotropic_spacing_and_attributes():
    dims, sp, org = (9, 12, 7), (0.5, 0.25, 1.0), (-1.0, 2.0, 0.5)
    x, y, z = nodes_xyz(org, sp, dims)
    f = (ISO + 1.4 - np.sqrt((x - 1.0) ** 2 + (y - 3.4) ** 2 * 4 + (z - 3.4) ** 2 / 1.5)).astype(np.float32)
    g = np.stack([x, y, z, f], 1).astype(np.float32)
    m = sm.extract(f, org, sp, dims, ISO, np.float32, {"g": g})
    chi, _ = sm.mesh_checks(m["vertices"], m["triangles"], closed=True, lattice_volume=4.0 * 2.75 * 6.0)
    assert chi == 2 and m["vertices"].dtype == np.float32
    # an attribute that IS the position interpolates to the vertex (up to rounding), and the interpolated density to iso
    assert np.abs(m["attrs"]["g"][:, :3] - m["vertices"][:, :3]).max() < 1e-5
    assert np.abs(m["attrs"]["g"][:, 3] - ISO).max() < 1e-5


def test_every_case_is_wound_by_geometry_and_pairs_up():
    """all 256 inside patterns of one cell inside a 4 x 4 x 4 lattice whose other nodes are outside: closed and oriented"""
    for bits in range(1, 256):
        f = np.zeros((4, 4, 4))
        for c in range(8):
            if (bits >> c) & 1:
                f[1 + ((c >> 2) & 1), 1 + ((c >> 1) & 1), 1 + (c & 1)] = 2.0
        m = sm.extract(f.ravel(), (0, 0, 0), 1.0, (4, 4, 4), ISO, np.float64)
        chi, _ = sm.mesh_checks(m["vertices"], m["triangles"], closed=True, lattice_volume=27.0)
        # (0 happens: the six corners off the body diagonal are a ring around it, as the diagonal's ends are outside)
        assert chi in (0, 2, 4, 6, 8), (bits, chi)
