"""Shared scene builders and comparison helpers for the parity tests."""
import numpy as np

from nereus_amd import capi, scene
from tests.oracle_lib import IISPH, SESPH, Oracle


def default_scene(solver=SESPH, double=False, kernel_set=1):
    """The reference's shipped scene: constructor defaults + generateParticleCube(center(-0.4,0.04,0.5), 0.5^3)
    (main.cpp:533-538).  SESPH: N=2197, IISPH: N=1331.  No boundaries."""
    p = Oracle.default_params(solver, double, kernel_set)
    pos = Oracle.generate_cube(p, [-0.4, 0.04, 0.5, 1.0], [0.5, 0.5, 0.5, 1.0], double, kernel_set)
    vel = np.zeros_like(pos)
    return p, pos, vel


def small_dam_break(lattice=(12, 10, 9), solver=SESPH, double=False, kernel_set=1, jitter=0.01):
    """A small dam-break with the 5-face boundary box; the grid comes from the updateGrid rule."""
    p = Oracle.default_params(solver, double, kernel_set)
    real = np.float64 if double else np.float32
    sc = scene.dam_break(lattice, h=float(p["interactionRadius"][0]), kpoly=float(p["kpoly"][0]), real=real,
                         jitter=jitter)
    return p, sc


def compressed_block(lattice=(10, 10, 10), solver=IISPH, double=False, kernel_set=1, ratio=0.72):
    """A jittered lattice at spacing ratio*h (< 0.794 h, i.e. denser than rest density) so the IISPH pressure
    solve has positive pressures to work on (the shipped scene is under-dense: all pressures clamp to 0)."""
    p = Oracle.default_params(solver, double, kernel_set)
    real = np.float64 if double else np.float32
    h = float(p["interactionRadius"][0])
    pos = scene.fluid_block(*lattice, h, real=real, jitter=0.02, spacing=ratio * h)
    return p, pos, np.zeros_like(pos)


def compressed_dam_break(lattice=(12, 10, 9), solver=IISPH, double=False, kernel_set=1, ratio=0.72):
    """small_dam_break's tank (5-face boundary box, grid from the updateGrid rule) holding a jittered lattice at spacing ratio*h
    instead of the resting one: the resting dam-break clamps every IISPH pressure to 0.  Returns (params, pos, vel, bi, vbi)."""
    p, sc = small_dam_break(lattice, solver=solver, double=double, kernel_set=kernel_set)
    real = np.float64 if double else np.float32
    pos = scene.fluid_block(*lattice, float(p["interactionRadius"][0]), real=real, jitter=0.02,
                            spacing=ratio * float(p["interactionRadius"][0]))
    return p, pos, np.zeros_like(pos), sc["bi"], sc["vbi"]


def rel_err(a, b):
    """max |a-b| / max|b| (array-level relative error, robust near zero entries)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = np.max(np.abs(b))
    if scale == 0:
        return float(np.max(np.abs(a - b)))
    return float(np.max(np.abs(a - b)) / scale)


def check_cell_tables(cs_a, ce_a, cs_b, ce_b):
    """cellStart bit-exact everywhere; cellEnd only where the cell is non-empty (stale elsewhere)."""
    np.testing.assert_array_equal(cs_a, cs_b)
    m = cs_b != 0xFFFFFFFF
    np.testing.assert_array_equal(ce_a[m], ce_b[m])


def next_sorted_keys(params, pos, real):
    """The `hash` (sorted cell keys) and `index` (stable argsort: the slot each sorted particle had in `pos`) that the step taken from
    the positions `pos` must show, whichever sort path the context takes: the coherent re-sort's merge and the full radix sort both
    claim this order.  pos: the positions the step starts from, in the context's order (a download after the step before); params:
    the context's; real: its SReal.  Built on diffuse_model's cells and sorted_order, whose power-of-two wrap is the reference's.  A cell
    coordinate that is NaN or outside int32 converts as the device's (int) does (NaN -> 0, saturating), which numpy's cast
    does not promise: those rows get their cells here and the stable sort is taken of the keys directly."""
    from tests import diffuse_model as dm  # (imports the smoothing-kernel models; only this helper needs them)

    gs = np.asarray(params["gridSize"]).reshape(-1)[:3].astype(np.int64)
    wo = np.asarray(params["worldOrigin"]).reshape(-1)[:3].astype(real)
    cs = np.asarray(params["cellSize"]).reshape(-1)[:3].astype(real)
    with np.errstate(invalid="ignore", over="ignore"):
        c = dm.cells(params, pos, real)
        q = np.floor((np.asarray(pos)[:, :3].astype(real) - wo) / cs)
    odd = ~(np.abs(q) < 2.0 ** 31)
    if odd.any():
        c[odd] = np.where(np.isnan(q[odd]), 0, np.where(q[odd] > 0, 2 ** 31 - 1, -2 ** 31))
        c &= gs - 1
        keys = (c[:, 2] * gs[1] + c[:, 1]) * gs[0] + c[:, 0]
        index = np.argsort(keys, kind="stable")
    else:
        c &= gs - 1
        keys = (c[:, 2] * gs[1] + c[:, 1]) * gs[0] + c[:, 0]
        index = dm.sorted_order(params, pos, real)
    return keys[index].astype(np.uint32), index.astype(np.uint32)


def close_masked(got, want, tol, what=""):
    """NaN-aware comparison: the non-finite entries are the same element for element (NaN where NaN, inf of the same sign), the
    finite ones are within `tol` array-relative.  Returns the error of the finite entries."""
    got, want = np.asarray(got), np.asarray(want)
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isfinite(got), fin, err_msg=what)
    np.testing.assert_array_equal(got[~fin], want[~fin], err_msg=what)   # (NaN == NaN here)
    e = rel_err(got[fin], want[fin]) if fin.any() else 0.0
    print("%s: %.3g (bar %.0e, %d non-finite)" % (what, e, tol, int((~fin).sum())))
    assert e <= tol, (what, e, tol)
    return e


# ---- the plate scene of the kinematic-body tests -------------------------------------------------------------------------------
SOLVERS = [capi.SESPH, capi.IISPH, capi.PCISPH, capi.PBF, capi.DFSPH]
SOLVER_NAMES = {capi.SESPH: "sesph", capi.IISPH: "iisph", capi.PCISPH: "pcisph", capi.PBF: "pbf", capi.DFSPH: "dfsph"}
PLATE_V = (9.0, 0.0, 0.0)            # two cell faces (2 h = 0.0914) in 11 steps of 1 ms
DOT_V, BAR_W = (0.5, 0.3, 0.0), (0.0, 0.0, 30.0)
_plate_cache = {}


def plate_scene(double=False, kernel_set=capi.MULLER, plate_gap=None, squeeze=1.0):
    """The scene of tests/test_bodies_gpu.py: small_dam_break moved three cells from the wall x = 0 inside its boundary box (body 0), a
    plate (body 1), a single particle (body 2) and a bar (body 3).  (params, pos, vel, bi, vbi, body_of, parts); plate_gap: distance
    of the plate from the fluid's first layer (default: the plate starts one spacing in front of the wall x = 0); squeeze < 1 contracts the fluid column towards its lower corner on the plate's
    side (the resting lattice is below rest density, and DFSPH's density solve would have nothing to do)"""
    key = (double, kernel_set, plate_gap, squeeze)
    if key in _plate_cache:
        return _plate_cache[key]
    real = np.float64 if double else np.float32
    p, sc = small_dam_break(double=double, kernel_set=kernel_set)
    h = float(p["interactionRadius"][0])
    d = h - 0.005
    pos = sc["pos"].copy()
    pos[:, 0] = (pos[:, 0].astype(np.float64) + 3.0 * h).astype(real)
    if squeeze != 1.0:
        lo = pos[:, :3].astype(np.float64).min(axis=0)
        pos[:, :3] = (lo + (pos[:, :3].astype(np.float64) - lo) * squeeze).astype(real)
    x0 = d if plate_gap is None else float(pos[:, 0].min()) - plate_gap

    def pts(a):
        o = np.ones((len(a), 4), real)
        o[:, :3] = np.asarray(a, np.float64).astype(real)
        return o

    jy, jz = np.meshgrid(np.arange(15), np.arange(11), indexing="ij")
    plate = pts(np.stack([np.full(jy.size, x0), (jy.ravel() + 1) * d, (jz.ravel() + 1) * d], axis=1))
    dot = pts([[0.9, 0.33, 0.21]])
    bar = pts(np.stack([0.7 + np.arange(7) * d, np.full(7, 0.4), np.full(7, 0.23)], axis=1))
    parts = [sc["bi"].astype(real), plate, dot, bar]
    bi = np.concatenate(parts)
    vbi = np.concatenate([sc["vbi"].astype(real)] + [capi.boundary_volumes(a, h, double=double) for a in parts[1:]])
    body_of = np.concatenate([np.full(len(a), k, np.uint32) for k, a in enumerate(parts)])
    assert len(bi) % 256 != 0 and len(bi) > 256
    _plate_cache[key] = (p, pos, sc["vel"].copy(), bi, vbi, body_of, parts)
    return _plate_cache[key]


def plate_solver(sc, solver, bodies=True, moving=True, plate_v=PLATE_V, **kw):
    """a Solver on plate_scene() with fixed iteration counts; bodies assigned, and moving, unless told otherwise"""
    p, pos, vel, bi, vbi, body_of, _ = sc
    s = capi.Solver(p, len(pos), solver=solver, **kw)
    s.set_particles(pos, vel)
    s.set_boundaries(bi, vbi, update_grid=True)
    if solver == capi.DFSPH:
        s.dfsph_configure(0.0, 3, 0.0, 3, 1)
    if solver == capi.PBF:
        s.pbf_configure(0.0, 3, 0.01, 0.0)
    if solver in (capi.PCISPH, capi.IISPH):
        s.set_max_iterations(4)
    if bodies:
        s.set_boundary_bodies(body_of, 4)
        if moving:
            s.set_body_velocity(1, plate_v)
            s.set_body_velocity(2, DOT_V)
            s.set_body_velocity(3, (0, 0, 0), BAR_W)
    return s
