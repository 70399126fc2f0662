"""The surface extraction on the device (include/nereus_hip.h "surface extraction"; DESIGN.md "Surface extraction") against the numpy
model of tests/surface_model.py, whose docstring says why the comparison is exact: V, T, the vertex and attribute bytes equal, the
triangles equal cell by cell as sets of cyclically normalised triples; and against mesh_checks, which needs no model.  The density
the model meshes is the sampler's own (nrs_sample_result after the extract): the sampler has its tests in tests/test_sample_gpu.py.
"""
import numpy as np
import pytest

from nereus_amd import capi
from tests import sample_model as spm
from tests import surface_model as sm
from tests.common import small_dam_break
from tests.test_sample_gpu import BUILD_IDS, BUILDS, dam_state, refused, tiny_grid_solver

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
D, G, VEL = capi.FIELD_DENSITY, capi.FIELD_GRADIENT, capi.FIELD_VELOCITY
ATTRS = capi.SURFACE_GRADIENT | capi.SURFACE_VELOCITY
MESH = [capi.MESH_VERTICES, capi.MESH_TRIANGLES, capi.MESH_GRADIENT, capi.MESH_VELOCITY]
NODES_PER_WORKGROUP = 256           # SURF_BLOCK of nrs_kernels_surface.h: the count, vertex and triangle kernels
NODES_PER_SCAN_PASS = 1024 * 256    # SCAN_BLOCK workgroup totals per pass of the one scanning workgroup


def fluid_lattice(pos, h, spacing, pad=2.0):
    """the fluid's bounding box inflated by pad * h (>= 2: every boundary node is farther than h from every particle, its density is 0)"""
    lo = pos[:, :3].astype(np.float64).min(0) - pad * h
    hi = pos[:, :3].astype(np.float64).max(0) + pad * h
    return tuple(float(x) for x in lo), tuple(int(np.ceil((hi[a] - lo[a]) / spacing)) + 1 for a in range(3))


def download(s, flags):
    m = {w: s.surface_result(w) for w in MESH[:2]}
    if flags & capi.SURFACE_GRADIENT:
        m[capi.MESH_GRADIENT] = s.surface_result(capi.MESH_GRADIENT)
    if flags & capi.SURFACE_VELOCITY:
        m[capi.MESH_VELOCITY] = s.surface_result(capi.MESH_VELOCITY)
    return m


def same_mesh(a, b, what):
    assert a.keys() == b.keys()
    for w in a:
        assert a[w].dtype == b[w].dtype and a[w].shape == b[w].shape and a[w].tobytes() == b[w].tobytes(), (what, "result %d differs" % w)


def extract_and_check(s, origin, spacing, dims, iso, flags, closed, what):
    """one extract against the model on the sampler's own arrays; returns (mesh, model, density)"""
    V, T = s.surface_extract(origin, spacing, dims, iso, flags)
    dens = s.sample_result(D)
    assert len(dens) == dims[0] * dims[1] * dims[2]
    attrs = {}
    if flags & capi.SURFACE_GRADIENT:
        attrs[capi.MESH_GRADIENT] = s.sample_result(G)
    if flags & capi.SURFACE_VELOCITY:
        attrs[capi.MESH_VELOCITY] = s.sample_result(VEL)
    want = sm.extract(dens, origin, spacing, dims, iso, s.real, attrs)
    print("%s: V %d T %d (model %d %d)" % (what, V, T, want["V"], want["T"]))
    assert (V, T) == (want["V"], want["T"]), what
    m = download(s, flags)
    assert m[capi.MESH_VERTICES].shape == (V, 4) and m[capi.MESH_TRIANGLES].shape == (T, 3)
    sm.compare(m[capi.MESH_VERTICES], m[capi.MESH_TRIANGLES], want, {w: m[w] for w in attrs}, what)
    sp = np.broadcast_to(np.asarray(spacing, np.float64), (3,))
    sm.mesh_checks(m[capi.MESH_VERTICES], m[capi.MESH_TRIANGLES], closed, float(np.prod((np.array(dims) - 1) * sp)))
    if closed:
        border = np.ones(dims[::-1], bool)
        border[1:-1, 1:-1, 1:-1] = False
        assert not dens.reshape(dims[::-1])[border].any()  # (the field is exactly 0 on the lattice boundary)
    return m, want, dens


def iso_of(p):
    return 0.5 * float(p["restDensity"][0])


# ---- 1. against the model, with both attributes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_against_model(double, ks):
    s, p, h, pos, vel, bs = dam_state(double, ks)
    origin, dims = fluid_lattice(pos, h, h / 2)
    s.sample_lattice(origin, h / 2, dims, D | G | VEL)
    before = {f: s.sample_result(f) for f in (D, G, VEL)}
    m, want, dens = extract_and_check(s, origin, h / 2, dims, iso_of(p), ATTRS, True, "model")
    for f in (D, G, VEL):  # the extract's sample call IS nrs_sample_lattice
        assert s.sample_result(f).tobytes() == before[f].tobytes()
    assert want["V"] > 200 and want["T"] > 400
    ptr, nbytes = s.surface_device_ptr(capi.MESH_TRIANGLES)
    assert ptr and nbytes == 12 * want["T"]
    assert s.surface_device_ptr(capi.MESH_VELOCITY)[1] == 4 * np.dtype(s.real).itemsize * want["V"]


# ---- 2. several workgroups, several passes of the scan -----------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_many_workgroups(double, ks):
    s, p, h, pos, vel, bs = dam_state(double, ks)
    origin, dims = fluid_lattice(pos, h, h / 6, pad=6.0)  # (padded evenly: the surface lies in the middle passes of the scan, behind a carry)
    dims = tuple(d | 1 for d in dims)
    if len(set(dims)) < 3:
        dims = (dims[0] + 4, dims[1] + 2, dims[2])
    nodes = dims[0] * dims[1] * dims[2]
    assert len(set(dims)) == 3 and all(d % 2 == 1 and d % 64 != 0 for d in dims)
    assert nodes >= 100000 and nodes >= 3 * NODES_PER_WORKGROUP and nodes >= 3 * NODES_PER_SCAN_PASS
    m, want, dens = extract_and_check(s, origin, h / 6, dims, iso_of(p), ATTRS, True, "many workgroups")
    assert want["V"] > 20000


# ---- 3. the smallest lattice: one corner inside ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_smallest_lattice(double, ks):
    real = np.float64 if double else np.float32
    s = None
    for c in range(8):
        if s is None:
            s, p, h = tiny_grid_solver(double, ks, 4, np.ones((1, 4), real))
        origin, spacing, dims = (1.5 * h,) * 3, 0.9 * h, (2, 2, 2)
        nodes = spm.lattice_points(origin, spacing, dims, real)
        s.set_particles(nodes[c:c + 1].copy(), np.zeros((1, 4), real))  # the particle ON corner c, bit for bit
        s.sample_lattice(origin, spacing, dims, D)
        dens = s.sample_result(D).astype(np.float64)
        others = np.delete(dens, c)
        assert dens[c] > 1.5 * others.max() and others.max() > 0  # (0.9 h: the axis neighbours see the particle, the diagonal ones do not)
        iso = 0.5 * (dens[c] + others.max())
        m, want, _ = extract_and_check(s, origin, spacing, dims, iso, ATTRS, False, "corner %d" % c)
        assert (want["V"], want["T"]) == ((7, 6) if c in (0, 7) else (4, 2))
        t = m[capi.MESH_VERTICES][:, 3]
        assert np.all(t > 0) and np.all(t < 1)
        # (corner 000 owns its seven edges; corner 111 is the far end of seven edges of seven owners)
        assert len(np.unique(m[capi.MESH_VERTICES][:, :3], axis=0)) == want["V"]
    s.close()


# ---- 4. cut by the lattice boundary ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_cut_by_the_boundary(double, ks):
    s, p, h, pos, vel, bs = dam_state(double, ks)
    origin, dims = fluid_lattice(pos, h, h / 2)
    dims = (dims[0] // 2, dims[1], dims[2])
    m, want, dens = extract_and_check(s, origin, h / 2, dims, iso_of(p), capi.SURFACE_GRADIENT, False, "cut")
    assert want["T"] > 200
    last = dens.reshape(dims[::-1])[:, :, -1]
    assert (last >= np.dtype(s.real).type(iso_of(p))).any()  # (the fluid does reach the cut)
    with pytest.raises(AssertionError):
        sm.mesh_checks(m[capi.MESH_VERTICES], m[capi.MESH_TRIANGLES], True)


# ---- 5. nodes exactly at the iso value ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_node_exactly_at_iso(double, ks):
    s, p, h, pos, vel, bs = dam_state(double, ks)
    origin, dims = fluid_lattice(pos, h, h / 2)
    s.sample_lattice(origin, h / 2, dims, D)
    dens = s.sample_result(D)
    # an interior-surface node of case 1: inside there, with an outside node at the other end of one of its 14 lattice edges; of those
    # the one with the smallest density, so that at iso = its density it is still inside and those neighbours are still outside
    f = dens.reshape(dims[::-1])
    ins = f >= np.dtype(s.real).type(iso_of(p))
    cand = np.zeros_like(ins)
    nx, ny, nz = dims
    for dx, dy, dz in sm.EDGE_DIRS:
        lo_, hi_ = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx)), (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        cand[lo_] |= ins[lo_] & ~ins[hi_]
        cand[hi_] |= ins[hi_] & ~ins[lo_]
    assert cand.sum() > 100
    q = int(np.argmin(np.where(cand.ravel(), dens.astype(np.float64), np.inf)))
    iso = float(dens[q])  # the SReal value as a double
    assert iso_of(p) <= iso < 1.7 * iso_of(p)
    m, want, dens2 = extract_and_check(s, origin, h / 2, dims, iso, ATTRS, True, "at iso")
    assert dens2.tobytes() == dens.tobytes()
    v = m[capi.MESH_VERTICES]
    x = spm.lattice_points(origin, h / 2, dims, s.real)[q]
    idx = (q % dims[0], (q // dims[0]) % dims[1], q // (dims[0] * dims[1]))
    assert all(0 < idx[a] < dims[a] - 1 for a in range(3))  # (an interior node)
    # the node is inside, so its edges towards outside nodes cross AT the node: t == 0 on the ones it owns (the vertex IS the node,
    # p0 + 0 * (p1 - p0)), t == (iso - f0) / (iso - f0) == 1 on those its lower neighbours own
    exact = (v[:, 3] == 0) | (v[:, 3] == 1)
    assert exact.sum() >= 1
    at_node = np.all(v[:, :3] == x[:3], axis=1)
    assert np.all(exact[at_node]) and np.all(at_node[v[:, 3] == 0])


# ---- 6. empty surfaces ---------------------------------------------------------------------------------------------------------------------
def assert_empty(s, flags):
    for w, cols in ((capi.MESH_VERTICES, 4), (capi.MESH_TRIANGLES, 3)):
        assert s.surface_result(w).shape == (0, cols)
        assert s.surface_device_ptr(w) == (None, 0)
    if flags & capi.SURFACE_GRADIENT:
        assert s.surface_result(capi.MESH_GRADIENT).shape == (0, 4)


@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_empty(double, ks):
    s, p, h, pos, vel, bs = dam_state(double, ks)
    origin, dims = fluid_lattice(pos, h, h / 2)
    s.sample_lattice(origin, h / 2, dims, D)
    top = float(s.sample_result(D).max())
    assert top > iso_of(p)
    assert s.surface_extract(origin, h / 2, dims, iso_of(p), ATTRS)[0] > 0  # (buffers that hold a mesh: the next results must not show it)
    assert s.surface_extract(origin, h / 2, dims, 1.001 * top, ATTRS) == (0, 0)  # iso above the lattice's maximum
    assert_empty(s, ATTRS)
    away = tuple(float(x) for x in pos[:, :3].astype(np.float64).max(0) + 3 * h)
    assert s.surface_extract(away, h / 2, (7, 5, 3), iso_of(p), 0) == (0, 0)     # a lattice away from the fluid
    assert not s.sample_result(D).any()
    assert_empty(s, 0)
    refused(s, E_STATE, lambda: s.surface_result(capi.MESH_GRADIENT))
    t, tp, th = tiny_grid_solver(double, ks, 4, np.ones((1, 4), s.real))
    t.set_particles(np.zeros((0, 4), s.real))                                        # a context without particles
    assert t.surface_extract((0.0, 0.0, 0.0), th / 2, (5, 4, 3), iso_of(tp), ATTRS) == (0, 0)
    assert_empty(t, ATTRS)
    t.close()


# ---- 7. with the wall term --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_walls(double, ks):
    s, p, h, pos, vel, bs = dam_state(double, ks)
    origin, dims = fluid_lattice(pos, h, h / 2)
    s.sample_lattice(origin, h / 2, dims, D)
    plain = s.sample_result(D)
    m, want, dens = extract_and_check(s, origin, h / 2, dims, iso_of(p), capi.SURFACE_WALLS | capi.SURFACE_GRADIENT, False, "walls")
    assert (dens > plain).any() and want["V"] > 200  # (the wall term is in the density the mesh was cut from)


# ---- 8. read-only, cached, and the mesher's buffers are its own ----------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [capi.SESPH, capi.DFSPH], ids=["sesph", "dfsph"])
def test_read_only_and_cached(solver):
    p, sc = small_dam_break((12, 10, 9))
    h = float(p["interactionRadius"][0])
    pair = []
    for k in range(2):
        s = capi.Solver(p, len(sc["pos"]), solver=solver)
        s.set_particles(sc["pos"], sc["vel"])
        s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
        pair.append(s)
    a, b = pair
    a.step(3)
    origin, dims = fluid_lattice(a.download()[0], h, h / 2)
    builds = a.sample_builds()
    V, T = a.surface_extract(origin, h / 2, dims, iso_of(p), ATTRS)
    assert V > 200 and a.sample_builds() == builds + 1
    first = download(a, ATTRS)
    assert a.surface_extract(origin, h / 2, dims, iso_of(p), ATTRS) == (V, T)
    same_mesh(first, download(a, ATTRS), "two extracts of one state")
    assert a.sample_builds() == builds + 1
    # the mesh survives the sampler's release and a later sample call
    a.sample_release()
    a.sample_points(np.ones((5, 4), np.float32), D)
    same_mesh(first, download(a, ATTRS), "after sample_release and sample_points")
    builds = a.sample_builds()
    a.step(2)
    b.step(5)
    for x, y in zip(a.download(pressure=True), b.download(pressure=True)):
        assert x.tobytes() == y.tobytes()
    V2, T2 = a.surface_extract(origin, h / 2, dims, iso_of(p), 0)
    assert a.sample_builds() == builds + 1 and V2 > 200
    assert a.surface_result(capi.MESH_VERTICES).tobytes() != first[capi.MESH_VERTICES].tobytes()
    a.surface_release()
    refused(a, E_STATE, lambda: a.surface_result(capi.MESH_VERTICES))
    assert len(a.sample_result(D)) == dims[0] * dims[1] * dims[2]  # (surface_release frees only the mesher's buffers)
    assert a.surface_extract(origin, h / 2, dims, iso_of(p), 0) == (V2, T2)
    a.close()
    b.close()


# ---- 9. refusals, each leaving the context usable ----------------------------------------------------------------------------------------------
def test_refusals():
    p, sc = small_dam_break((12, 10, 9))
    h = float(p["interactionRadius"][0])
    iso = iso_of(p)
    s = capi.Solver(p, len(sc["pos"]), solver=capi.SESPH)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    origin, dims = fluid_lattice(sc["pos"], h, h / 2)
    for w in MESH:  # before any extract
        refused(s, E_STATE, lambda: s.surface_result(w))
        refused(s, E_STATE, lambda: s.surface_device_ptr(w))
    good = s.surface_extract(origin, h / 2, dims, iso, capi.SURFACE_GRADIENT)
    mesh = download(s, capi.SURFACE_GRADIENT)
    assert good[0] > 200

    def usable():
        assert s.surface_extract(origin, h / 2, dims, iso, capi.SURFACE_GRADIENT) == good
        same_mesh(mesh, download(s, capi.SURFACE_GRADIENT), "after a refusal")

    refused(s, E_STATE, lambda: s.surface_result(capi.MESH_VELOCITY))      # an attribute the last extract did not compute
    refused(s, E_STATE, lambda: s.surface_device_ptr(capi.MESH_VELOCITY))
    for w in (0, 3, 16, 15, 1 << 31):                                      # not exactly one result id
        refused(s, E_INVALID, lambda: s.surface_result(w))
        refused(s, E_INVALID, lambda: s.surface_device_ptr(w))
    for bad in (0.0, -iso, np.nan, np.inf, -np.inf):
        refused(s, E_INVALID, lambda: s.surface_extract(origin, h / 2, dims, bad, 0))
    for flags in (8, 16, 7 | 8, 1 << 31):
        refused(s, E_INVALID, lambda: s.surface_extract(origin, h / 2, dims, iso, flags))
    for d in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (512, 512, 513), (2 ** 27 + 1, 2, 2), (2048, 2048, 513), (65536, 65536, 2)):
        refused(s, E_INVALID, lambda: s.surface_extract(origin, h / 2, d, iso, 0))
    for spacing in (0.0, -h, np.nan, np.inf, (h, h, 0.0)):
        refused(s, E_INVALID, lambda: s.surface_extract(origin, spacing, dims, iso, 0))
    refused(s, E_INVALID, lambda: s.surface_extract((0.0, np.nan, 0.0), h / 2, dims, iso, 0))
    refused(s, E_INVALID, lambda: s._chk(s.lib.nrs_surface_extract(s.h, None, iso, 0, None, None)))
    usable()
    L = capi.Solver._lattice(origin, h / 2, dims)
    s._chk(s.lib.nrs_surface_extract(s.h, L, iso, capi.SURFACE_GRADIENT, None, None))  # the out pointers may be NULL
    same_mesh(mesh, download(s, capi.SURFACE_GRADIENT), "NULL out pointers")
    # mid-update after a partial step
    s.step_partial(capi.STAGE_DENSITY)
    refused(s, E_STATE, lambda: s.surface_extract(origin, h / 2, dims, iso, 0))
    same_mesh(mesh, download(s, capi.SURFACE_GRADIENT), "a refused extract keeps the last mesh")
    s.set_particles(sc["pos"], sc["vel"])
    usable()
    # a grid the sampler refuses
    base = s.params
    for name, val in (("cellSize", (0.9 * h, h, h)), ("gridSize", (2, 64, 64)), ("gridSize", (64, 48, 64))):
        bad = base.copy()
        bad[name][0] = val
        bad["numCells"][0] = int(np.prod(bad["gridSize"][0]))
        s.set_params(bad)
        refused(s, E_INVALID, lambda: s.surface_extract(origin, h / 2, dims, iso, 0))
        s.set_params(base)
        usable()
    s.surface_release()
    for w in MESH:
        refused(s, E_STATE, lambda: s.surface_result(w))
        refused(s, E_STATE, lambda: s.surface_device_ptr(w))
    s.surface_release()  # (twice is fine)
    usable()
    # a slab context
    s.slab_configure(0, 64, 8)
    refused(s, E_INVALID, lambda: s.surface_extract(origin, h / 2, dims, iso, 0))
    s.close()
    # a host-driven IISPH step in progress
    p2, sc2 = small_dam_break((12, 10, 9), solver=capi.IISPH)
    t = capi.Solver(p2, len(sc2["pos"]), solver=capi.IISPH)
    t.set_particles(sc2["pos"], sc2["vel"])
    t.set_boundaries(sc2["bi"], sc2["vbi"], update_grid=True)
    t.iisph_predict()
    refused(t, E_STATE, lambda: t.surface_extract(origin, h / 2, dims, iso, 0))
    t.iisph_iterate()
    t.iisph_finish()
    assert t.surface_extract(origin, h / 2, dims, iso_of(p2), 0)[0] > 200
    t.close()
