"""Scenes and CPU-side helpers shared by tests/test_slab_builds_gpu.py (the device) and tests/test_slab_bars_cpu.py (the yardsticks):
a helper module, not a test.  Everything here runs on the CPU: the scenes, the oracle's states, the cell-x crossings of a run and
the distance of the nearest pair from the cut-off radius."""
import numpy as np

from nereus_amd import slab
from tests.common import compressed_dam_break
from tests.oracle_lib import IISPH, SESPH, Oracle

BUILDS = [(False, 1), (False, 0), (True, 1), (True, 0)]   # (double, kernel set): capi.MULLER = 1, capi.MONAGHAN = 0
BUILD_IDS = ["f32-muller", "f32-monaghan", "f64-muller", "f64-monaghan"]
SESPH_LATTICE = (27, 8, 7)
SESPH_HALO = slab.HALO_CELLS
PER_SIDE = 3   # particles put on either side of every deciding face
# The block stands 0.15 h further from the three walls it starts at than its own spacing: its outer layers are 0.95 h from the wall
# planes, inside the walls' reach but not pressed against them.  Pressed (0.8 h), the wall forces are ten times every other force
# and set the scale of the array-relative error: a one-cell halo then costs the fp32 Monaghan forces only 40x the stage bar, and
# the oracle's own order sensitivity of the fp32 Muller forces is a third of it, where a tenth is asked for
# (tests/test_slab_bars_cpu.py prints both; the fp32 force sensitivity is 0.8e-7 to 2.4e-7 for every gap between 0.10 and 0.21 h,
# at 0.15 h it is 1.6e-7 and 0.9e-7 in the two kernel sets).
WALL_GAP = 0.15
_cache = {}


def tait_of(double):
    """the oracle's Tait mode that the device of this precision is compared with (tests/test_parity_gpu.py)"""
    return "double7" if double else "powf"


def grid_params(p, double, kset, solver, bi, vbi):
    """the parameters after the updateGrid rule has seen the tank: what every rank and the single domain are created with"""
    o = Oracle(p, double, kset, solver)
    o.set_boundaries(bi, vbi, update_grid=True)
    return o.params


def faces_of(cuts, halo):
    """the cell faces that decide something for an interior cut c: those of cells c - H, c - 1, c, c + 1, c + H"""
    return sorted({c + k for c in cuts for k in (-halo, -1, 0, 1, halo)})


def sesph_scene(double, kset):
    """A block of 27 x 8 x 7 particles at spacing 0.8 h, jitter 0.02, in small_dam_break's tank with walls (WALL_GAP): about 21 cells
    long in x, several particles per cell.  Ids ride in vel.w, x velocities alternate +-2.5 m/s.  Cuts for two and for three slabs; on every
    face that decides something for one of those cuts (faces_of) the nearest particles are moved onto the face: PER_SIDE that move
    right to the largest x below it, PER_SIDE that move left onto it.  Returns a dict; the arrays are shared, do not write to them."""
    key = ("sesph", double, kset)
    if key in _cache:
        return _cache[key]
    real = np.float64 if double else np.float32
    nx, ny, nz = SESPH_LATTICE
    p, pos, vel, bi, vbi = compressed_dam_break(SESPH_LATTICE, solver=SESPH, double=double, kernel_set=kset, ratio=0.8)
    p = grid_params(p, double, kset, SESPH, bi, vbi)
    pos = pos.copy()
    pos[:, :3] += real(WALL_GAP * float(p["interactionRadius"][0]))
    n = len(pos)
    gid = np.arange(n)
    vel = np.zeros_like(pos)
    vel[:, 0] = np.where(((gid // nz) % ny + gid % nz) % 2 == 0, 2.5, -2.5).astype(real)
    vel[:, 3] = gid.astype(real)
    ox, cs = real(p["worldOrigin"][0][0]), real(p["cellSize"][0][0])
    cx = slab.cell_of(pos[:, 0], ox, cs, real)
    c_lo, c_hi = int(cx.min()), int(cx.max()) + 1
    w = c_hi - c_lo
    assert w >= 20, w
    cuts2 = [slab.NO_CUT_LO, c_lo + w // 2, slab.NO_CUT_HI]
    cuts3 = [slab.NO_CUT_LO, c_lo + w // 3, c_lo + (2 * w) // 3, slab.NO_CUT_HI]
    taken = np.zeros(n, bool)
    on_face = 0
    for f in faces_of(cuts2[1:-1] + cuts3[1:-1], SESPH_HALO):
        xf = real(ox + cs * real(f))
        # the face as the device sees it: the smallest x whose cell is f
        while slab.cell_of([xf], ox, cs, real)[0] >= f:
            xf = np.nextafter(xf, real(-np.inf))
        while slab.cell_of([xf], ox, cs, real)[0] < f:
            xf = np.nextafter(xf, real(np.inf))
        dist = np.abs(pos[:, 0].astype(np.float64) - float(xf)) + np.where(taken, 1e9, 0.0)
        below = np.argsort(dist + np.where(vel[:, 0] > 0, 0.0, 1e9))[:PER_SIDE]   # (moving right: they cross the face in the first step)
        at = np.argsort(dist + np.where(vel[:, 0] < 0, 0.0, 1e9))[:PER_SIDE]      # (moving left: so do these)
        pos[below, 0] = np.nextafter(xf, real(-np.inf))
        pos[at, 0] = xf
        taken[below] = taken[at] = True
        assert np.all(slab.cell_of(pos[below, 0], ox, cs, real) == f - 1) and np.all(slab.cell_of(pos[at, 0], ox, cs, real) == f)
        on_face += 2 * PER_SIDE
    sc = dict(p=p, pos=pos, vel=vel, bi=bi, vbi=vbi, n=n, real=real, cuts={2: cuts2, 3: cuts3}, on_face=on_face,
              h=float(p["interactionRadius"][0]))
    _cache[key] = sc
    return sc


def by_id(pos, vel):
    o = np.argsort(vel[:, 3].astype(np.int64), kind="stable")
    return pos[o], vel[o]


def oracle_states(double, kset, steps, sc=None, key=None, threads=1):
    """[(pos, vel) by id after t steps, t = 0 .. steps] of the single-domain oracle on the scene (default: sesph_scene)"""
    key = ("states", key or "sesph", double, kset, steps)
    if key in _cache:
        return _cache[key]
    sc = sc or sesph_scene(double, kset)
    o = Oracle(sc["p"], double, kset, SESPH, tait=tait_of(double), threads=threads)
    o.set_particles(sc["pos"], sc["vel"])
    o.set_boundaries(sc["bi"], sc["vbi"], update_grid=False)
    out = [by_id(sc["pos"], sc["vel"])]
    for _ in range(steps):
        o.step(1)
        out.append(by_id(o.get("pos").copy(), o.get("vel").copy()))
    _cache[key] = out
    return out


def crossings(states, cuts, p, real):
    """how many times a particle's cell-x moved across an interior cut between two consecutive states (by id)"""
    ox, cs = p["worldOrigin"][0][0], p["cellSize"][0][0]
    cxs = [slab.cell_of(s[0][:, 0], ox, cs, real) for s in states]
    total = 0
    for a, b in zip(cxs[:-1], cxs[1:]):
        for c in cuts[1:-1]:
            total += int(((a < c) != (b < c)).sum())
    return total


def cut_off_margin(states, h):
    """min | |r_ij| - h | over all pairs within 1.05 h and all states: how far the nearest pair is from flipping the decision
    r < h of the truncated Monaghan kernels (which do not vanish at h)"""
    from scipy.spatial import cKDTree

    best = np.inf
    for pos, _ in states:
        x = np.asarray(pos[:, :3], np.float64)
        pairs = cKDTree(x).query_pairs(1.05 * h, output_type="ndarray")
        if len(pairs):
            r = np.linalg.norm(x[pairs[:, 0]] - x[pairs[:, 1]], axis=1)
            best = min(best, float(np.abs(r - h).min()))
    return best


# ---- IISPH ---------------------------------------------------------------------------------------------------------------------
IISPH_LATTICE = (22, 8, 8)


def iisph_scene(double, kset, walls):
    """the compressed block of tests/test_slab_gloo.py's _iisph_scene in the given build, x velocities +-1.5 m/s.  Without walls:
    spacing 0.72 h (Monaghan 0.58 h, as tests.common.compressed_block) under the IISPH constructor defaults (128^3 grid).  With
    walls: in small_dam_break's tank, spacing 0.72 h for both kernel sets and the outer layers 0.99 h from the wall planes: the
    tank's grid is 16 cells high and deep, and the Monaghan block at 0.58 h, or pressed against the walls, throws particles out of
    it within two steps (the oracle itself then differs between a slab with its halo and the whole domain: inside_grid is the
    precondition).  Returns (params, pos, vel, bi, vbi)."""
    key = ("iisph", double, kset, walls)
    if key in _cache:
        return _cache[key]
    from nereus_amd import scene

    real = np.float64 if double else np.float32
    if walls:
        p, pos, vel, bi, vbi = compressed_dam_break(IISPH_LATTICE, solver=IISPH, double=double, kernel_set=kset, ratio=0.72)
        p = grid_params(p, double, kset, IISPH, bi, vbi)
        pos = pos.copy()
        pos[:, :3] += real((0.99 - 0.72) * float(p["interactionRadius"][0]))
    else:
        p = Oracle.default_params(IISPH, double, kset)
        h = float(p["interactionRadius"][0])
        pos = scene.fluid_block(*IISPH_LATTICE, h, real=real, jitter=0.02, spacing=(0.72 if kset == 1 else 0.58) * h)
        bi = vbi = None
    vel = np.zeros_like(pos)
    vel[:, 0] = np.where((np.arange(len(pos)) // IISPH_LATTICE[2]) % 2 == 0, 1.5, -1.5).astype(real)
    _cache[key] = (p, pos, vel, bi, vbi)
    return _cache[key]


def iisph_oracle_positions(double, kset, walls, steps, min_iters=2):
    """positions of the by-slot oracle on iisph_scene before each of `steps` steps and after the last"""
    key = ("iisph-states", double, kset, walls, steps, min_iters)
    if key not in _cache:
        p, pos, vel, bi, vbi = iisph_scene(double, kset, walls)
        o = Oracle(p, double, kset, IISPH, self_by_slot=True, tait="double7")
        o.set_particles(pos, vel)
        o.set_boundaries(bi, vbi, update_grid=False)
        out = [pos]
        for _ in range(steps):
            o.step(1, max_iters=-min_iters if min_iters != 2 else 0)
            out.append(o.get("pos").copy())
        _cache[key] = out
    return _cache[key]


def inside_grid(positions, p, margin=1):
    """every particle of every state is at least `margin` cells inside the grid on every axis (outside it the cell hash wraps)"""
    org, cs, gs = p["worldOrigin"][0], p["cellSize"][0], p["gridSize"][0].astype(np.int64)
    for pos in positions:
        c = np.floor((np.asarray(pos[:, :3], np.float64) - org) / cs)
        if not (np.isfinite(c).all() and (c >= margin).all() and (c < gs - margin).all()):
            return False
    return True
