"""The numpy model of the anisotropic surface reconstruction (tests/aniso_model.py) on shapes whose answer is known, and the claim the
feature rests on: on the under-dense dam break the iso-surface of the raw SPH density is a foam of closed surfaces, that of the
anisotropic colour field one closed surface of genus 0 (DESIGN.md "Anisotropic kernels")."""
import numpy as np

from tests import aniso_model as am
from tests import sample_model as spm
from tests import surface_model as sm
from tests.common import small_dam_break

H = 0.0457


def test_one_particle_is_a_sphere():
    x = np.array([[0.1, -0.2, 0.3]])
    r = am.records(x, H, np.float64, support=0.8 * H, k_n=0.4)
    assert r["count"][0] == 1
    np.testing.assert_array_equal(r["center"][0], x[0])
    np.testing.assert_allclose(r["axes"][0], 0.4 * 0.8 * H, rtol=1e-15)
    np.testing.assert_allclose(r["G"][0], np.eye(3) / (0.32 * H), rtol=1e-14, atol=1e-12)
    assert r["bound"][0] == r["axes"][0].max()
    # the volume-normalised weight: V = 1 / (k6 r^6) for the one neighbour at distance 0
    rr = 2 * H
    np.testing.assert_allclose(r["weight"][0], am.K315 * (64 * np.pi * rr ** 9 / 315 / rr ** 6) / (0.32 * H) ** 3, rtol=1e-13)


def test_flat_sheet_is_a_disc():
    i, j = np.meshgrid(np.arange(17), np.arange(17), indexing="ij")
    x = np.stack([i.ravel() * H / 2, j.ravel() * H / 2, np.full(i.size, 0.25)], axis=1)
    r = am.records(x, H, np.float64, support=H / 2)
    c = 8 * 17 + 8
    assert r["count"][c] >= 25
    a = np.sort(r["axes"][c])[::-1]
    np.testing.assert_allclose(a[0], a[1], rtol=1e-9)
    np.testing.assert_allclose(a[0] / a[2], 4.0, rtol=1e-9)
    np.testing.assert_allclose(r["center"][c], x[c], atol=1e-12)
    # the short axis is the sheet's normal: G n = n / a3, and G t = t / a1 in the sheet
    np.testing.assert_allclose(r["G"][c] @ [0, 0, 1], np.array([0, 0, 1]) / a[2], atol=1e-6 / H)
    np.testing.assert_allclose(r["G"][c] @ [1, 0, 0], np.array([1, 0, 0]) / a[0], atol=1e-6 / H)
    assert a.max() < 1.5 * H


def test_line_is_a_needle():
    # (spacing h / 4 as nearly as keeps no particle AT the distance 2 h, where rounding would decide its membership: 0.26 h, 7 each side)
    x = np.stack([np.arange(41) * 0.26 * H, np.full(41, 0.1), np.full(41, -0.3)], axis=1)
    r = am.records(x, H, np.float64, support=H / 2, n_eps=5)
    a = np.sort(r["axes"][20])[::-1]
    assert r["count"][20] == 15
    np.testing.assert_allclose([a[0] / a[1], a[0] / a[2]], 4.0, rtol=1e-9)
    np.testing.assert_allclose(r["G"][20] @ [1, 0, 0], np.array([1, 0, 0]) / a[0], atol=1e-6 / H)
    assert a.max() < 1.5 * H
    # with the default n_eps = 25 the same particle keeps the sphere
    s = am.records(x, H, np.float64, support=H / 2)
    np.testing.assert_allclose(s["axes"][20], 0.25 * H, rtol=1e-15)


def test_rotating_the_particles_rotates_g():
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 6 * H, (160, 3))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    a, b = am.records(x, H, np.float64), am.records(x @ q.T, H, np.float64)
    np.testing.assert_array_equal(a["count"], b["count"])
    assert (a["count"] >= 25).sum() > 20 and (a["count"] < 25).sum() > 20  # (ellipsoids and spheres)
    np.testing.assert_allclose(b["G"], np.einsum("ik,nkl,jl->nij", q, a["G"], q), rtol=0, atol=1e-9 / H)
    np.testing.assert_allclose(b["center"], a["center"] @ q.T, rtol=0, atol=1e-12)
    np.testing.assert_allclose(b["weight"], a["weight"], rtol=1e-10)


def test_one_closed_surface_where_the_density_gives_a_foam():
    p, sc = small_dam_break((12, 10, 9))
    h = float(p["interactionRadius"][0])
    pos = sc["pos"]
    real = pos.dtype.type
    origin, dims = am.padded_lattice(pos, h, h / 2, 2.5)
    assert dims == (31, 28, 26)
    nodes = spm.lattice_points(origin, h / 2, dims, real)
    r = am.records(pos, h, real)
    f = am.field(r["center"], r["bound"], r["G"], r["weight"], None, nodes, real)
    mesh = sm.extract(f["phi"].astype(real), origin, h / 2, dims, 0.5, real)
    chi, vol = sm.mesh_checks(mesh["vertices"], mesh["triangles"], True)
    comps = am.components(mesh["triangles"], mesh["V"])
    rho = am.poly6_density(pos, nodes, h, float(p["kpoly"][0]), float(p["particleMass"][0]))
    raw = sm.extract(rho.astype(real), origin, h / 2, dims, 0.5 * float(p["restDensity"][0]), real)
    sm.mesh_checks(raw["vertices"], raw["triangles"], True)
    raw_comps = am.components(raw["triangles"], raw["V"])
    print("anisotropic: %d component(s), chi %d, volume %.4f; raw density: %d components" % (comps, chi, vol, raw_comps))
    assert comps == 1 and chi == 2
    assert raw_comps >= 10
    border = np.ones(dims[::-1], bool)
    border[1:-1, 1:-1, 1:-1] = False
    assert not f["phi"].reshape(dims[::-1])[border].any()
