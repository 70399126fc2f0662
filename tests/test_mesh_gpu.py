"""Mesh sampling on the device (include/nereus_hip.h "mesh sampling"; DESIGN.md "Mesh sampling") against the numpy model
(tests/mesh_model.py) on the cases of tests/test_mesh_model_cpu.py, where the model alone shows that they are not vacuous and that no
node lies in the band |w - 0.5| < 1e-6 (so the device's selection must equal the model's node for node).

dist2, nearest and closest3 are IEEE-exact: byte-equal.  The winding number goes through atan2, whose inputs are bit-identical on both
sides: a <= 2 ulp device atan2 and a <= 1 ulp host atan2 on values <= pi differ by at most 2.1e-16 per term in units of w, one
differing rounding of a running sum <= 4 pi * few adds 1.4e-16, together <= 2^-51 per triangle; the bar |w - w_model| <= T * 2^-48
leaves a factor 8.

nrs_emit_mesh is checked like nrs_emit_block (tests/test_inflow_gpu.py): a twin context receives the model's selection through
nrs_upload_particles(first = n), then both step, and n and the downloads must be byte-equal.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from nereus_amd import capi
from tests import mesh_model as mm
from tests.common import small_dam_break
from tests.test_inflow_gpu import CASE_IDS, CASES, E_CAPACITY, E_INVALID, E_STATE, pair, refused, same_state

pytestmark = pytest.mark.gpu

S = mm.S
INSIDE, OUTSIDE, SNAP = capi.MESH_INSIDE, capi.MESH_OUTSIDE, capi.MESH_SNAP
EXACT = ("dist2", "nearest", "closest")


def w_bar(nt):
    return nt * 2.0 ** -48


def check_field(got, want, nt, what, winding=True):
    for k in EXACT:
        assert got[k].tobytes() == want[k].tobytes(), (what, k, int((got[k] != want[k]).sum()))
    if winding:
        err = np.abs(got["winding"] - want["winding"]).max()
        print("%s: max |w - w_model| = %.3g (bar %.3g)" % (what, err, w_bar(nt)))
        assert err <= w_bar(nt), (what, err)


# ---- 1. the field against the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mm.CASES)
def test_field_matches_model(name):
    v, t, o, s, d = mm.case(name)
    want = mm.case_field(name)
    got = capi.mesh_field(v, t, o, s, d)
    assert not np.isnan(got["dist2"]).any()
    check_field(got, want, len(t), name)
    # bit-reproducible from run to run
    again = capi.mesh_field(v, t, o, s, d)
    for k in got:
        assert again[k].tobytes() == got[k].tobytes(), k
    # a subset of the outputs: the same bytes (the winding alone and the distance alone are kernels of their own)
    for ask in (dict(winding=True, dist2=False, nearest=False, closest=False), dict(winding=False, dist2=True, nearest=False, closest=False),
                dict(winding=False, dist2=False, nearest=True, closest=False), dict(winding=False, dist2=False, nearest=False, closest=True),
                dict(winding=True, dist2=False, nearest=True, closest=False)):
        part = capi.mesh_field(v, t, o, s, d, **ask)
        assert sorted(part) == sorted(k for k in ask if ask[k])
        for k in part:
            assert part[k].tobytes() == got[k].tobytes(), (ask, k)


# ---- 2. shapes at which the kernel can go wrong ----------------------------------------------------------------------------------------------------
TORUS = mm.case("torus")
SHAPE_T = sorted(set([1, mm.UNROLL - 1, mm.UNROLL, mm.UNROLL + 1, 2 * mm.UNROLL + 3]))


@pytest.mark.parametrize("nt", SHAPE_T)
def test_triangle_counts_around_the_unroll_width(nt):
    v, t, o, s, d = TORUS
    t = t[:nt]  # (the mesh need not be closed: the model is the reference)
    got = capi.mesh_field(v, t, o, s, d)
    check_field(got, mm.lattice_field(v, t, o, s, d), nt, "T = %d" % nt)
    assert (got["nearest"] < nt).all()


@pytest.mark.parametrize("dims,origin", [((1, 1, 1), (0.05, 0.06, 0.02)), ((65, 1, 1), (-0.19, 0.013, 0.004)), ((1, 65, 1), (0.11, -0.19, 0.004)),
                                         ((3, 1, 67), (0.1, 0.0, -0.3))],
                         ids=["one-node", "65x1x1", "1x65x1", "3x1x67"])
def test_small_lattices(dims, origin):
    v, t = TORUS[:2]
    got = capi.mesh_field(v, t, origin, (S, 0.5 * S, 0.25 * S), dims)
    check_field(got, mm.lattice_field(v, t, origin, (S, 0.5 * S, 0.25 * S), dims), len(t), str(dims))


def test_node_on_a_vertex_and_on_a_face():
    v, t = mm.case("cube")[:2]
    lo, hi = mm.CUBE_LO, mm.CUBE_HI
    on_vertex = tuple(v[5])
    on_face = (lo[0], 0.5 * (lo[1] + hi[1]) + 0.01, 0.5 * (lo[2] + hi[2]) - 0.02)
    for what, origin in (("vertex", on_vertex), ("face", on_face)):
        got = capi.mesh_field(v, t, origin, S, (1, 1, 1))
        want = mm.lattice_field(v, t, origin, S, (1, 1, 1))
        check_field(got, want, len(t), what, winding=False)
        assert np.isfinite(got["winding"]).all()
        # the vertex is its own closest point; on the face the in-plane coordinates come out of the barycentric sum, rounded
        assert got["dist2"][0] == 0.0 if what == "vertex" else got["dist2"][0] < 1e-30
        assert np.abs(got["closest"] - np.array([origin])).max() <= (0.0 if what == "vertex" else 1e-15)


def test_triangle_with_two_equal_indices():
    v, t, o, s, d = mm.case("cube")
    t = np.concatenate([t[:5], np.array([[1, 1, 5], [2, 6, 6], [3, 3, 3]], np.uint32), t[5:]])
    got = capi.mesh_field(v, t, o, s, d)
    assert not np.isnan(got["dist2"]).any() and not np.isnan(got["closest"]).any()
    want = mm.lattice_field(v, t, o, s, d)
    check_field(got, want, len(t), "degenerate")
    # the triangles without area lie on the cube's edges and corners: no node comes closer to them than to the cube
    assert np.abs(got["dist2"] - mm.case_field("cube")["dist2"]).max() < 1e-15


# ---- 3. two batches: 168 x 160 x 160 = 4,300,800 nodes > 2^22 -----------------------------------------------------------------------------------------
BIG_DIMS, BIG_S = (168, 160, 160), 0.004
BIG_ORIGIN = (-0.23, -0.25, 0.17 - 156 * BIG_S)  # node 2^22 lies in the plane k = 156, which cuts the cube
BIG_MARGIN = 0.012


@functools.lru_cache(maxsize=None)
def big_candidates():
    """The nodes within BIG_MARGIN of the cube's bounding box (linear indices, positions) and the model's field there.  Every other
    node is farther than BIG_MARGIN from the mesh (the mesh lies in its bounding box) and outside the closed cube (winding 0)."""
    v, t = mm.case("cube")[:2]
    ax = [np.float64(BIG_ORIGIN[a]) + np.arange(BIG_DIMS[a], dtype=np.float64) * BIG_S for a in range(3)]
    near = [np.nonzero((ax[a] > mm.CUBE_LO[a] - BIG_MARGIN) & (ax[a] < mm.CUBE_HI[a] + BIG_MARGIN))[0] for a in range(3)]
    k, j, i = np.meshgrid(near[2], near[1], near[0], indexing="ij")
    q = ((k * BIG_DIMS[1] + j) * BIG_DIMS[0] + i).ravel()
    P = np.stack([ax[0][i.ravel()], ax[1][j.ravel()], ax[2][k.ravel()]], axis=1)
    return q, P, mm.field(v, t, P)


@pytest.mark.parametrize("flags,dmin,dmax", [(INSIDE | OUTSIDE, 0.0, 1.5 * BIG_S), (INSIDE, 1.5 * BIG_S, np.inf)], ids=["shell", "fill"])
def test_two_batches_particles(flags, dmin, dmax):
    v, t = mm.case("cube")[:2]
    assert BIG_DIMS[0] * BIG_DIMS[1] * BIG_DIMS[2] == 4300800 > mm.BATCH
    q, P, f = big_candidates()
    assert (np.diff(q) > 0).all() and np.abs(f["winding"] - 0.5).min() >= 1e-6
    assert dmax < BIG_MARGIN or flags == INSIDE  # (what the candidates leave out cannot be selected)
    want = mm.particles(f, P, flags, dmin, dmax, np.float32)
    mask = mm.selected(f, flags, dmin, dmax)
    assert (q[mask] < mm.BATCH).sum() > 1000 and (q[mask] >= mm.BATCH).sum() > 1000  # both batches contribute
    got = capi.mesh_particles(v, t, BIG_ORIGIN, BIG_S, BIG_DIMS, flags=flags, dmin=dmin, dmax=dmax)
    assert len(got) == len(want) and got.tobytes() == want.tobytes()


def test_two_batches_field_tail():
    v, t = mm.case("cube")[:2]
    got = capi.mesh_field(v, t, BIG_ORIGIN, BIG_S, BIG_DIMS, winding=False, nearest=False, closest=False)["dist2"]
    total = len(got)
    want = mm.field(v, t, mm.nodes(BIG_ORIGIN, BIG_S, BIG_DIMS, first=total - 1000, count=1000), winding=False)["dist2"]
    assert got[-1000:].tobytes() == want.tobytes()
    # and around the seam between the batches
    seam = mm.field(v, t, mm.nodes(BIG_ORIGIN, BIG_S, BIG_DIMS, first=mm.BATCH - 500, count=1000), winding=False)["dist2"]
    assert got[mm.BATCH - 500:mm.BATCH + 500].tobytes() == seam.tobytes()


# ---- 4. the selection ---------------------------------------------------------------------------------------------------------------------------
RULES = {"fill": (INSIDE, S, np.inf), "shell": (INSIDE | OUTSIDE, 0.0, S / 2), "snapped-shell": (INSIDE | OUTSIDE | SNAP, 0.0, S / 2)}


@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("name", mm.CASES)
def test_selection_matches_model(name, rule, double):
    v, t, o, s, d = mm.case(name)
    flags, dmin, dmax = RULES[rule]
    real = np.float64 if double else np.float32
    want = mm.particles(mm.case_field(name), mm.nodes(o, s, d), flags, dmin, dmax, real)
    assert 0 < len(want) < d[0] * d[1] * d[2]
    assert capi.mesh_particles(v, t, o, s, d, flags=flags, dmin=dmin, dmax=dmax, double=double, count_only=True) == len(want)
    got = capi.mesh_particles(v, t, o, s, d, flags=flags, dmin=dmin, dmax=dmax, double=double)
    assert got.dtype == real and got.shape == want.shape and got.tobytes() == want.tobytes()


def test_selection_sides_and_nothing():
    v, t, o, s, d = mm.case("torus")
    f, P = mm.case_field("torus"), mm.nodes(o, s, d)
    for flags, dmin, dmax in ((OUTSIDE, 0.0, S / 2), (OUTSIDE, 0.0, np.inf), (INSIDE, 0.0, np.inf), (INSIDE | OUTSIDE, 0.0, np.inf), (INSIDE | SNAP, 0.0, np.inf)):
        want = mm.particles(f, P, flags, dmin, dmax, np.float32)
        got = capi.mesh_particles(v, t, o, s, d, flags=flags, dmin=dmin, dmax=dmax)
        assert len(want) > 0 and got.tobytes() == want.tobytes(), (flags, dmin, dmax)
    assert capi.mesh_particles(v, t, o, s, d, flags=INSIDE, dmin=10.0, count_only=True) == 0
    assert capi.mesh_particles(v, t, o, s, d, flags=INSIDE, dmin=10.0).shape == (0, 4)


def test_selection_capacity():
    v, t, o, s, d = mm.case("icosphere")
    lib = capi.load_library()
    M, keep = capi._mesh(v, t)
    L = capi._lattice(o, s, d)
    R = capi._mesh_rule(INSIDE, S, np.inf)
    count = C.c_uint64(0)
    n = 358
    buf = np.full((n + 4, 4), -77.0, np.float32)
    assert lib.nrs_mesh_particles(-1, 32, C.byref(M), C.byref(L), C.byref(R), capi._ptr(buf), n - 1, C.byref(count)) == E_CAPACITY
    assert count.value == n and (buf == -77.0).all() and b"capacity" in lib.nrs_last_error()
    assert lib.nrs_mesh_particles(-1, 32, C.byref(M), C.byref(L), C.byref(R), capi._ptr(buf), n, C.byref(count)) == 0
    assert count.value == n and (buf[n:] == -77.0).all() and (buf[:n, 3] == 1.0).all()
    assert lib.nrs_mesh_particles(-1, 32, C.byref(M), C.byref(L), C.byref(R), None, 0, C.byref(count)) == 0 and count.value == n
    assert lib.nrs_mesh_particles(-1, 32, C.byref(M), C.byref(L), C.byref(R), capi._ptr(buf), 1 << 40, None) == 0  # (count may be NULL)


def test_refusals_of_the_context_free_calls():
    v, t, o, s, d = mm.case("cube")
    for call in (lambda **kw: capi.mesh_field(**kw), lambda **kw: capi.mesh_particles(**kw)):
        base = dict(vertices=v, triangles=t, origin=o, spacing=s, dims=d)
        for kw in (dict(vertices=np.zeros((0, 3))), dict(triangles=np.zeros((0, 3), np.uint32)), dict(triangles=np.array([[0, 1, 8]], np.uint32)),
                   dict(vertices=np.where(np.arange(24).reshape(8, 3) == 7, np.nan, v)), dict(spacing=0.0), dict(dims=(4, 0, 4)), dict(origin=(0.0, np.inf, 0.0))):
            refused(E_INVALID, lambda: call(**dict(base, **kw)))
    for kw in (dict(flags=0), dict(flags=SNAP), dict(flags=9), dict(dmin=-1.0), dict(dmin=np.nan), dict(dmax=np.nan), dict(dmin=0.2, dmax=0.1)):
        refused(E_INVALID, lambda: capi.mesh_particles(v, t, o, s, d, **kw))
    lib = capi.load_library()
    M, keep = capi._mesh(v, t)
    L, R = capi._lattice(o, s, d), capi._mesh_rule(INSIDE, 0.0, np.inf)
    count = C.c_uint64(5)
    assert lib.nrs_mesh_particles(-1, 16, C.byref(M), C.byref(L), C.byref(R), None, 0, C.byref(count)) == E_INVALID and b"precision" in lib.nrs_last_error()
    assert lib.nrs_mesh_particles(-1, 32, None, C.byref(L), C.byref(R), None, 0, C.byref(count)) == E_INVALID
    assert lib.nrs_mesh_particles(-1, 32, C.byref(M), None, C.byref(R), None, 0, C.byref(count)) == E_INVALID
    assert lib.nrs_mesh_particles(-1, 32, C.byref(M), C.byref(L), None, None, 0, C.byref(count)) == E_INVALID
    assert lib.nrs_mesh_particles(-1, 32, C.byref(M), C.byref(L), C.byref(capi._mesh_rule(INSIDE, 0.0, 1.0, reserved=1)), None, 0, C.byref(count)) == E_INVALID
    assert lib.nrs_mesh_field(-1, None, C.byref(L), None, None, None, None) == E_INVALID
    assert lib.nrs_mesh_field(-1, C.byref(M), C.byref(L), None, None, None, None) == 0  # nothing asked for


# ---- 5. nrs_emit_mesh: the icosphere fill into an empty context and into the air above the dam -----------------------------------------------------------
SHIFT = np.array([0.25, 0.65, 0.2])
FILL = (INSIDE, S, np.inf)


@functools.lru_cache(maxsize=None)
def emit_case():
    """the icosphere case moved to where the tank of small_dam_break((12, 10, 9)) has air, with the model's field there"""
    v, t, o, s, d = mm.case("icosphere")
    v, o = v + SHIFT, tuple(np.asarray(o) + SHIFT)
    f = mm.lattice_field(v, t, o, s, d)
    assert np.abs(f["winding"] - 0.5).min() >= 1e-6  # (the condition of the selection tests, on the moved case)
    return v, t, o, s, d, f


def model_fill(real, vel):
    v, t, o, s, d, f = emit_case()
    pos = mm.particles(f, mm.nodes(o, s, d), *FILL, real)
    v4 = np.zeros_like(pos)
    v4[:, :3] = np.asarray(vel, real)
    return pos, v4


@pytest.mark.parametrize("solver,double,ks", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("fluid", [False, True], ids=["empty", "dam"])
def test_emit_mesh(solver, double, ks, fluid):
    v, t, o, s, d, f = emit_case()
    vel = (0.25, -0.5, 0.125)
    pos, v4 = model_fill(np.float64 if double else np.float32, vel)
    m = len(pos)
    assert 300 < m < 400
    p0, sc = small_dam_break((12, 10, 9), double=double, kernel_set=ks, solver=solver)
    assert pos[:, 1].min() > sc["pos"][:, 1].max() + 0.5 * float(p0["interactionRadius"][0])  # in the air above the dam
    sa, tw, p, sc = pair(solver, double, ks, scene=(p0, sc), capacity=(1080 if fluid else 0) + m + 50, fluid=fluid)  # (room for one fill, not for two)
    n0 = sa.n
    assert sa.emit_mesh(v, t, o, s, d, *FILL, vel=vel) == m and sa.n == n0 + m
    tw.set_particles(pos, v4, first=n0)
    same_state(sa, tw, "after the fill")
    assert sa.download()[0][n0:].tobytes() == pos.tobytes()
    for k in range(3):
        sa.step(1)
        tw.step(1)
        same_state(sa, tw, "step %d" % k)
    # all or nothing
    before = sa.download(pressure=True)
    refused(E_CAPACITY, lambda: sa.emit_mesh(v, t, o, s, d, *FILL, vel=vel))
    assert sa.n == n0 + m and all(a.tobytes() == b.tobytes() for a, b in zip(before, sa.download(pressure=True)))
    sa.close()
    tw.close()


def test_emit_mesh_tracked():
    v, t, o, s, d, f = emit_case()
    m = len(model_fill(np.float32, (0, 0, 0))[0])
    sa, tw, p, sc = pair(capi.SESPH, False, capi.MULLER, capacity=1080 + 2 * m)
    sa.track_enable(0)
    sa.step(2)
    assert sa.track_info() == (True, 0, 1080)
    assert sa.emit_mesh(v, t, o, s, d, *FILL) == m
    ids, births = sa.track_result(capi.TRACK_ID), sa.track_result(capi.TRACK_BIRTH)
    assert ids[1080:].tolist() == list(range(1080, 1080 + m)) and (births[1080:] == 2).all() and (births[:1080] == 0).all()
    assert sorted(ids[:1080].tolist()) == list(range(1080)) and sa.track_info() == (True, 0, 1080 + m)
    sa.step(1)
    assert sa.emit_mesh(v, t, o, s, d, INSIDE, 2 * S, np.inf) > 0
    assert (sa.track_result(capi.TRACK_BIRTH)[1080 + m:] == 3).all() and sa.track_result(capi.TRACK_ID)[1080 + m] == 1080 + m
    sa.close()
    tw.close()


def test_emit_mesh_refusals():
    v, t, o, s, d, f = emit_case()
    p, sc = small_dam_break((12, 10, 9))
    sa = capi.Solver(p, len(sc["pos"]) + 357)  # one short of the fill
    sa.set_particles(sc["pos"], sc["vel"])
    sa.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    before = sa.download(pressure=True)

    def unchanged():
        return sa.n == 1080 and all(a.tobytes() == b.tobytes() for a, b in zip(before, sa.download(pressure=True)))
    refused(E_CAPACITY, lambda: sa.emit_mesh(v, t, o, s, d, *FILL))
    assert unchanged()
    refused(E_INVALID, lambda: sa.emit_mesh(v, t, o, s, d, INSIDE | SNAP, 0.0, S))
    refused(E_INVALID, lambda: sa.emit_mesh(v, t, o, s, d, INSIDE | OUTSIDE | SNAP, 0.0, S / 2))
    refused(E_INVALID, lambda: sa.emit_mesh(v, t, o, s, d, 0, 0.0, S))
    refused(E_INVALID, lambda: sa.emit_mesh(v, t, o, s, d, INSIDE, S, 0.0))
    refused(E_INVALID, lambda: sa.emit_mesh(v, t[:0], o, s, d, *FILL))
    refused(E_INVALID, lambda: sa.emit_mesh(v, t, o, 0.0, d, *FILL))
    refused(E_INVALID, lambda: sa.emit_mesh(v, t, o, s, d, *FILL, vel=(0, np.nan, 0)))
    refused(E_INVALID, lambda: sa._chk(sa.lib.nrs_emit_mesh(sa.h, None, None, None, None, None)))
    assert unchanged()
    assert sa.emit_mesh(v, t, o, s, d, INSIDE, 10.0, np.inf) == 0 and unchanged()  # a rule that selects nothing adds nothing
    # mid-update after a partial step
    sa.step_partial(capi.STAGE_DENSITY)
    refused(E_STATE, lambda: sa.emit_mesh(v, t, o, s, d, INSIDE, 3 * S, np.inf))
    sa.set_particles(sc["pos"], sc["vel"])
    assert unchanged()
    # a slab context
    sa.slab_configure(0, 64, 8)
    refused(E_INVALID, lambda: sa.emit_mesh(v, t, o, s, d, INSIDE, 3 * S, np.inf))
    sa.close()


# ---- 6. the path to walls: snapped shell -> Akinci volumes -> boundaries of a context --------------------------------------------------------------------
def test_snapped_shell_makes_a_wall():
    v, t, o, s, d = mm.case("torus")
    shell = capi.mesh_particles(v, t, o, s, d, flags=INSIDE | OUTSIDE | SNAP, dmin=0.0, dmax=S / 2)
    p, _ = small_dam_break((12, 10, 9), solver=capi.PCISPH)
    h = float(p["interactionRadius"][0])
    vbi = capi.boundary_volumes(shell, h)
    assert np.isfinite(vbi).all() and (vbi > 0).all()
    # a block of fluid in the torus's hole: it falls (gravity -y) onto the inside of the ring
    g = np.arange(-1, 2) * 0.8 * h
    x, y, z = np.meshgrid(g + 0.001, g + 0.002, g[:2] * 0.5 + 0.003, indexing="ij")
    pos = np.ones((x.size, 4), np.float32)
    pos[:, :3] = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    sa = capi.Solver(p, len(pos), solver=capi.PCISPH)
    vel = np.zeros_like(pos)
    vel[:, 1] = -1.0
    sa.set_particles(pos, vel)
    sa.set_boundaries(shell, vbi, update_grid=True)
    sa.step(20)
    out = sa.download()[0]
    sa.close()
    assert np.isfinite(out).all()
    for row in out.astype(np.float64):
        f = capi.mesh_field(v, t, row[:3], S, (1, 1, 1), nearest=False, closest=False)
        assert not (f["dist2"][0] < (0.25 * S) ** 2 and f["winding"][0] > 0.5), row
