"""Slab steps with real neighbours in all four builds (precision x kernel set, each its own instantiation unit), both kernel paths:
density with ghosts, forces, integrate, next keys and the classification for the next partition, and the IISPH chain over slabs,
against a single-domain context of the same build and flags on bit-identical inputs (only the order of the sums inside a cell
differs), and for the large cases against the oracle of the same build.  The ranks are contexts of this process
(tests/slab_ranks.py); the scenes and their CPU-checked preconditions are in tests/slab_scenes.py; the bars are those of
tests/test_parity_gpu.py, shown by tests/test_slab_bars_cpu.py to sit at least 10x above the oracle's own order sensitivity on these
scenes and at least 100x below what a one-cell halo or ignored ghosts would cost.  No particle is left out of any comparison."""
import os

import numpy as np
import pytest

from nereus_amd import capi, scene, slab
from tests import slab_scenes as S
from tests.common import rel_err
from tests.oracle_lib import SESPH, Oracle
from tests.slab_ranks import GHOST, HALO_L, HALO_R, MIG_L, MIG_R, SlabRanks
from tests.test_parity_gpu import TOL_STAGE, TOL_STAGE_F64, TOL_STEPS, TOL_STEPS_F64

pytestmark = pytest.mark.gpu

PATHS = pytest.mark.parametrize("ref", [False, True], ids=["tiled", "reforder"])
ALL_BUILDS = pytest.mark.parametrize("double,kset", S.BUILDS, ids=S.BUILD_IDS)
LOCKSTEP_STEPS = 6
_single = {}


def stage_bar(double):
    return TOL_STAGE_F64 if double else TOL_STAGE


def name(double, kset, ref):
    return "%s %s %s" % ("f64" if double else "f32", "muller" if kset == capi.MULLER else "monaghan", "reforder" if ref else "tiled")


def single_domain(sc, double, kset, ref, solver=capi.SESPH, flags=0):
    s = capi.Solver(sc["p"], 2 * sc["n"], solver=solver, double=double, kernel_set=kset, reference_order=ref, flags=flags)
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=False)
    return s


def single_stage(double, kset, ref, which):
    """density and forces by id of the single domain at state `which` of the oracle's run: computed once per build and path"""
    key = (double, kset, ref, which)
    if key not in _single:
        sc = S.sesph_scene(double, kset)
        pos, vel = S.oracle_states(double, kset, 4)[which]
        s = single_domain(sc, double, kset, ref)
        try:
            s.set_particles(pos, vel)
            s.step_partial(capi.STAGE_FORCES)
            ids = s.get("sortedVel")[:, 3].astype(np.int64)
            assert np.array_equal(np.sort(ids), np.arange(sc["n"]))
            dens, forces = np.empty(sc["n"], sc["real"]), np.empty((sc["n"], 4), sc["real"])
            dens[ids], forces[ids] = s.get("dens")[:sc["n"]], s.get("forces")[:sc["n"]]
        finally:
            s.close()
        assert np.isfinite(dens).all() and np.isfinite(forces).all() and dens.min() > 0
        _single[key] = (dens, forces)
    return _single[key]


def sesph_ranks(sc, world, double, kset, ref):
    return SlabRanks(sc["p"], sc["cuts"][world], S.SESPH_HALO, 2 * sc["n"], sc["n"], double=double, kernel_set=kset,
                     reference_order=ref)


def check_crossings(double, kset, world, steps):
    """on the CPU, before the device is looked at: particles change their owner during the run"""
    sc = S.sesph_scene(double, kset)
    states = S.oracle_states(double, kset, max(steps, 4))[:steps + 1]
    assert S.crossings(states, sc["cuts"][world], sc["p"], sc["real"]) > 0
    return sc


@pytest.mark.parametrize("world", [2, 3])
@PATHS
@ALL_BUILDS
def test_stage_windows_density_and_forces(hip_lib, double, kset, ref, world):
    """step_partial(STAGE_FORCES) on every rank after one exchange, at the upload state (particles on both sides of every deciding
    face) and at the oracle's state four steps later (drifted, several per cell).  Slot by slot: density equals the single domain's
    (stage bar) for every id with cell-x in [lo - 1, hi + 1) and is exactly 0 elsewhere; forces likewise for [lo, hi); every id is
    active for forces on exactly one rank."""
    sc = check_crossings(double, kset, world, 4)
    bar, n = stage_bar(double), sc["n"]
    worst = [0.0, 0.0]
    for which in (0, 4):
        pos, vel = S.oracle_states(double, kset, 4)[which]
        ref_dens, ref_forces = single_stage(double, kset, ref, which)
        R = sesph_ranks(sc, world, double, kset, ref)
        try:
            R.load(pos, vel, sc["bi"], sc["vbi"])
            counts = R.exchange()
            R.step_partial(capi.STAGE_FORCES)
            active = np.zeros(n, np.int64)
            for r, s in enumerate(R.ranks):
                lo, hi = R.cuts[r], R.cuts[r + 1]
                m = s.n
                left, right = (counts[r - 1] if r else None), (counts[r + 1] if r < world - 1 else None)
                arrived = (left[MIG_R] if left else 0) + (right[MIG_L] if right else 0)
                copies = (left[HALO_R] if left else 0) + (right[HALO_L] if right else 0)
                assert s.n_owned == counts[r][0] + arrived and m == s.n_owned + counts[r][GHOST] + copies and copies > 0
                sp, sv = s.get("sortedPos")[:m], s.get("sortedVel")[:m]
                dens, forces = s.get("dens")[:m], s.get("forces")[:m]
                assert len(sp) == len(dens) == len(forces) == m
                ids, cx = sv[:, 3].astype(np.int64), R.cell_x(sp[:, 0])
                in_d, in_f = (cx >= lo - 1) & (cx < hi + 1), (cx >= lo) & (cx < hi)
                assert (~in_d).sum() > 0 and (in_d & ~in_f).sum() > 0 and in_f.sum() == s.n_owned   # all three kinds of slot exist
                assert np.all(sp[in_f, 3] == 1) and np.all(sp[~in_f, 3] == 2)                      # halo copies are ghosts
                assert np.all(dens[~in_d] == 0), "density of an inactive halo copy"
                assert np.all(forces[~in_f] == 0), "forces of an inactive slot"
                e_d = rel_err(dens[in_d], ref_dens[ids[in_d]])
                e_f = rel_err(forces[in_f], ref_forces[ids[in_f]])
                worst = [max(worst[0], e_d), max(worst[1], e_f)]
                assert e_d <= bar and e_f <= bar, (which, r, e_d, e_f, bar)
                active += np.bincount(ids[in_f], minlength=n)
            assert np.all(active == 1), "every particle is active for forces on exactly one rank"
        finally:
            R.close()
    print("slab stage %s world %d: dens %.3g forces %.3g (bar %.0e)" % (name(double, kset, ref), world, worst[0], worst[1], bar))


@pytest.mark.parametrize("world", [2, 3])
@PATHS
@ALL_BUILDS
def test_lockstep_steps_equal_single_domain(hip_lib, double, kset, ref, world):
    """Six steps.  Before each one the union of the owned particles (a permutation of all ids) is uploaded into the single-domain
    context; both sides step once from these identical bits; the next union equals the single domain's download by id within the
    stage bar, every particle included (within a step both sides take the same cut-off decisions, Monaghan too).  The device's
    counts show migrants and halo copies on both sides of the middle slab."""
    sc = check_crossings(double, kset, world, LOCKSTEP_STEPS)
    bar, n = stage_bar(double), sc["n"]
    R = sesph_ranks(sc, world, double, kset, ref)
    s = single_domain(sc, double, kset, ref)
    worst = [0.0, 0.0]
    try:
        R.load(sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
        want = None
        for t in range(LOCKSTEP_STEPS + 1):
            R.exchange()
            pos, vel = S.by_id(*R.union())
            assert np.array_equal(vel[:, 3].astype(np.int64), np.arange(n)), "ids are a permutation of all ids"
            if want is not None:
                e_p, e_v = rel_err(pos[:, :3], want[0][:, :3]), rel_err(vel[:, :3], want[1][:, :3])
                worst = [max(worst[0], e_p), max(worst[1], e_v)]
                assert e_p <= bar and e_v <= bar, (t, e_p, e_v, bar)
            if t == LOCKSTEP_STEPS:
                break
            s.set_particles(pos, vel)
            s.step(1)
            R.step()
            want = S.by_id(*s.download())
        tot = R.totals
        mid = world // 2
        assert tot[mid - 1][MIG_R] > 0 and tot[mid][MIG_L] > 0 and tot[mid - 1][HALO_R] > 0 and tot[mid][HALO_L] > 0, tot
        if world == 3:
            assert tot[1][MIG_R] > 0 and tot[2][MIG_L] > 0 and tot[1][HALO_R] > 0 and tot[2][HALO_L] > 0, tot
        assert tot[:, GHOST].sum() > 0   # leavers that stay in the halo were kept as ghosts
    finally:
        R.close()
        s.close()
    print("slab lockstep %s world %d: pos %.3g vel %.3g (bar %.0e)" % (name(double, kset, ref), world, worst[0], worst[1], bar))


# ---- IISPH ---------------------------------------------------------------------------------------------------------------------
def _single_iisph_step(s, real, min_iters):
    """one step of the single domain: the library's own loop, or (more iterations than the reference's exit test asks for) the
    host-driven phases under the same rule as the slabs"""
    if min_iters == 2:
        s.step(1)
        return s.last_iterations
    s.iisph_predict()
    it, rho_avg = 0, real(0)
    while (float(rho_avg) - 1000.0) > 1.0 or it < min_iters:
        tot, cnt = s.iisph_iterate()
        rho_avg = slab.mean_density(tot, cnt, real)
        it += 1
    s.iisph_finish()
    return it


@pytest.mark.parametrize("walls,halo,min_iters", [(False, 8, 2), (True, 8, 2), (False, 12, 4)], ids=["nowall", "walls", "4iters-halo12"])
@PATHS
@ALL_BUILDS
def test_iisph_lockstep_by_slot(hip_lib, double, kset, ref, walls, halo, min_iters):
    """The IISPH chain over two slabs (NRS_FLAG_IISPH_SELF_BY_SLOT: the default self-exclusion depends on the order by design), four
    steps in lockstep with the single domain: the union with its pressures is uploaded before every step; iteration counts equal;
    particles paired by position; positions and velocities within the bars of this path (fp32 1e-5 / 1e-4, fp64 TOL_STEPS_F64).
    fp32 Muller is the control; with walls iisph_tail<true> runs on a slab; four iterations need the 12-cell halo.  Precondition,
    checked on the oracle's run: every step starts with all particles inside the grid (tests/slab_scenes.py iisph_scene)."""
    from scipy.spatial import cKDTree

    p, pos0, vel0, bi, vbi = S.iisph_scene(double, kset, walls)
    real, n = pos0.dtype.type, len(pos0)
    # on the CPU, before the device is looked at: every step starts with all particles inside the grid
    assert S.inside_grid(S.iisph_oracle_positions(double, kset, walls, 4, min_iters)[:4], p)
    tol_p, tol_v = (TOL_STEPS_F64, TOL_STEPS_F64) if double else (TOL_STEPS, 10 * TOL_STEPS)
    cx = slab.cell_of(pos0[:, 0], p["worldOrigin"][0][0], p["cellSize"][0][0], real)
    cuts = [slab.NO_CUT_LO, int(np.median(cx)) + 1, slab.NO_CUT_HI]
    flags = capi.FLAG_IISPH_SELF_BY_SLOT
    R = SlabRanks(p, cuts, halo, 4 * n, 2 * n, double=double, kernel_set=kset, solver=capi.IISPH, reference_order=ref, flags=flags)
    s = capi.Solver(p, 2 * n, solver=capi.IISPH, double=double, kernel_set=kset, reference_order=ref, flags=flags)
    worst = [0.0, 0.0, 0.0]
    try:
        s.set_boundaries(bi, vbi, update_grid=False)
        R.load(pos0, vel0, bi, vbi)
        want = None
        for t in range(5):
            R.exchange()
            pos, vel, pres = R.union()
            assert len(pos) == n and np.isfinite(pos).all() and np.isfinite(vel).all() and np.isfinite(pres).all()
            if want is not None:
                d, idx = cKDTree(want[0][:, :3]).query(pos[:, :3])
                assert len(np.unique(idx)) == n and d.max() < 1e-5, d.max()
                e = [rel_err(pos[:, :3], want[0][idx, :3]), rel_err(vel[:, :3], want[1][idx, :3]), rel_err(pres, want[2][idx])]
                worst = [max(a, b) for a, b in zip(worst, e)]
                assert e[0] <= tol_p and e[1] <= tol_v, (t, e, tol_p, tol_v)
                assert (want[2] > 0).any()   # a solve that clamps every pressure to 0 would check nothing
            if t == 4:
                break
            s.set_particles(pos, vel, pres)
            it_single = _single_iisph_step(s, real, min_iters)
            it_slabs = R.iisph_step(min_iters)
            assert it_single == it_slabs >= min_iters, (t, it_single, it_slabs)
            want = s.download(pressure=True)
        assert R.truncated_steps == 0
        assert R.totals[0][MIG_R] + R.totals[1][MIG_L] > 0 and R.totals[0][HALO_R] > 0 and R.totals[1][HALO_L] > 0, R.totals
    finally:
        R.close()
        s.close()
    print("slab iisph %s %s halo %d: pos %.3g vel %.3g pressure %.3g (bars %.0e / %.0e)"
          % (name(double, kset, ref), "walls" if walls else "nowall", halo, worst[0], worst[1], worst[2], tol_p, tol_v))


# ---- the in-place and pre-classified partition under fp64 ----------------------------------------------------------------------
BIG_LATTICE, BIG_STEPS = (48, 28, 26), 8
_big = {}


def big_scene(kset):
    """Two ranks of 48 x 28 x 26 particles each (above the 32,768 from which the partition works in place and the steps merge), fp64,
    the dam-break lattice of slab.rank_scene with x velocities +-2.5 m/s and ids in vel.w; the oracle's states of 8 steps."""
    if kset in _big:
        return _big[kset]
    real, world = np.float64, 2
    nx, ny, nz = BIG_LATTICE
    base = Oracle.default_params(SESPH, True, kset)
    shares = [slab.rank_scene(BIG_LATTICE, r, world, base, real=real) for r in range(world)]
    p, cuts = shares[0][0], shares[0][1]
    h = float(p["interactionRadius"][0])
    full = scene.dam_break((nx * world, ny, nz), h=h, kpoly=float(p["kpoly"][0]), real=real)
    n = nx * world * ny * nz
    pos = full["pos"]
    gid = np.arange(n)
    vel = np.zeros_like(pos)
    vel[:, 0] = np.where(((gid // nz) % ny + gid % nz) % 2 == 0, 2.5, -2.5)
    vel[:, 3] = gid
    cx = slab.cell_of(pos[:, 0], p["worldOrigin"][0][0], p["cellSize"][0][0], real)
    for r in range(world):   # the split by cell is rank_scene's
        assert np.array_equal(pos[(cx >= cuts[r]) & (cx < cuts[r + 1])], shares[r][2])
        assert len(shares[r][2]) > 32768
    sc = dict(p=p, pos=pos, vel=vel, bi=full["bi"], vbi=full["vbi"], n=n, real=real, cuts={2: cuts}, h=h)
    o = Oracle(p, True, kset, SESPH, tait="double7", threads=min(16, os.cpu_count() or 1))
    o.set_particles(pos, vel)
    o.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    np.testing.assert_array_equal(o.params.view(np.uint8), p.view(np.uint8))   # the global grid of rank_scene is the updateGrid rule's
    states = [S.by_id(pos, vel)]
    for _ in range(BIG_STEPS):
        o.step(1)
        states.append(S.by_id(o.get("pos").copy(), o.get("vel").copy()))
    sc["states"] = states
    sc["margin"] = S.cut_off_margin(states, h)
    _big[kset] = sc
    return sc


@pytest.mark.parametrize("recut", [False, True], ids=["fixed-cuts", "recut-after-4"])
@pytest.mark.parametrize("kset", [capi.MULLER, capi.MONAGHAN], ids=["f64-muller", "f64-monaghan"])
def test_partition_forms_fp64_end_state(hip_lib, kset, recut):
    """fp64, two ranks above 32,768 local particles, 8 steps with no download in between (the holes of the in-place partition are
    consumed by the coherent re-sort): the partition is pre-classified by the fused force kernel (NRS_STAT_SLAB_PARTITION 2) while
    the cuts stand and compacting (0) right after a one-cell re-cut; most steps merge.  The final union equals the single-domain
    device run and the oracle by id within TOL_STEPS_F64.  Precondition, checked first on the oracle's states: no pair comes closer
    than 1e-11 m to the cut-off radius (about 1e4 x the fp64 order sensitivity; the truncated Monaghan kernels jump there)."""
    sc = big_scene(kset)
    print("slab big f64 %s: min | |r| - h | over 8 steps %.3g m" % ("muller" if kset else "monaghan", sc["margin"]))
    assert sc["margin"] >= 1e-11, sc["margin"]
    cuts, n = sc["cuts"][2], sc["n"]
    assert S.crossings(sc["states"], cuts, sc["p"], sc["real"]) > 0
    msg_cap, ctx_cap = slab.capacities(BIG_LATTICE, sc["h"], n // 2, real=np.float64)
    R = SlabRanks(sc["p"], cuts, S.SESPH_HALO, ctx_cap, msg_cap, double=True, kernel_set=kset)
    s = capi.Solver(sc["p"], n, double=True, kernel_set=kset)
    try:
        R.load(sc["pos"], sc["vel"], sc["bi"], sc["vbi"])
        routes = []
        for t in range(BIG_STEPS):
            if recut and t == 4:
                R.set_cut(1, cuts[1] + 1)
            R.exchange()
            routes.append([int(q.get_stat(capi.STAT_SLAB_PARTITION)) for q in R.ranks])
            R.step()
        want_routes = [[0, 0]] + [[0, 0] if (recut and t == 4) else [2, 2] for t in range(1, BIG_STEPS)]
        assert routes == want_routes, routes
        for q in R.ranks:
            used, fallbacks = q.resort_stats()
            # every step after an in-place partition goes through the coherent re-sort (the first step and the one after the re-cut
            # sort from scratch); a fall-back is legitimate in a slab this narrow (tests/test_slab_gloo.py), most steps must merge
            assert used >= BIG_STEPS - (2 if recut else 1) and fallbacks <= used // 3, (used, fallbacks)
        R.exchange()
        pos, vel = S.by_id(*R.union())
        assert np.array_equal(vel[:, 3].astype(np.int64), np.arange(n))
        assert R.totals[0][MIG_R] + R.totals[1][MIG_L] > 0 and R.totals[0][HALO_R] > 0 and R.totals[1][HALO_L] > 0
        s.set_particles(sc["pos"], sc["vel"])
        s.set_boundaries(sc["bi"], sc["vbi"], update_grid=False)
        s.step(BIG_STEPS)
        dp, dv = S.by_id(*s.download())
        op, ov = sc["states"][BIG_STEPS]
        e = [rel_err(pos[:, :3], dp[:, :3]), rel_err(vel[:, :3], dv[:, :3]), rel_err(pos[:, :3], op[:, :3]), rel_err(vel[:, :3], ov[:, :3])]
        print("slab big f64 %s %s: vs single domain pos %.3g vel %.3g, vs oracle pos %.3g vel %.3g (bar %.0e)"
              % ("muller" if kset else "monaghan", "recut" if recut else "fixed", e[0], e[1], e[2], e[3], TOL_STEPS_F64))
        assert max(e) <= TOL_STEPS_F64, e
    finally:
        R.close()
        s.close()
