"""The bars of tests/test_slab_builds_gpu.py, judged on the CPU (oracle against oracle) on that file's own scenes.
1. Yardstick: a slab and the single domain differ only in the order of the particles inside a cell, so the oracle is run against
   itself on permutations of its input; the spread is at most a tenth of every bar used, and it is not zero (a scene with one
   particle per cell has no in-cell order and would be a blind yardstick).
2. The device tests can fail: the two likeliest bugs of a slab step (a halo one cell too narrow, ghosts ignored), modelled on the
   oracle, move the forces next to the cut by at least 100x the stage bar at the worse of the stage test's two states, 10x at each.
3. The fp64 bars tell an fp64 build from an fp32 one on these scenes by at least 100x (the pattern of tests/test_precision_bars.py)."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from nereus_amd import slab
from tests import slab_scenes as S
from tests.common import rel_err
from tests.oracle_lib import IISPH, SESPH, STOP_FORCES, Oracle
from tests.test_parity_gpu import TOL_STAGE, TOL_STAGE_F64, TOL_STEPS, TOL_STEPS_F64

ALL_BUILDS = pytest.mark.parametrize("double,kset", S.BUILDS, ids=S.BUILD_IDS)
PERMUTATIONS = 5


def _oracle(sc, double, kset, pos, vel, solver=SESPH, by_slot=False, pres=None):
    o = Oracle(sc["p"], double, kset, solver, tait=S.tait_of(double), self_by_slot=by_slot)
    o.set_particles(pos, vel, pres)
    o.set_boundaries(sc["bi"], sc["vbi"], update_grid=False)
    return o


def _stage(sc, double, kset, pos, vel):
    """(dens, forces) by id after one partial step"""
    o = _oracle(sc, double, kset, pos, vel)
    o.step(1, stop=STOP_FORCES)
    ids = o.get("sortedVel")[:, 3].astype(np.int64)
    dens, forces = np.empty(len(ids), o.real), np.empty((len(ids), 4), o.real)
    dens[ids], forces[ids] = o.get("dens"), o.get("forces")
    return dens, forces


def _steps(sc, double, kset, pos, vel, k):
    o = _oracle(sc, double, kset, pos, vel)
    o.step(k)
    return S.by_id(o.get("pos").copy(), o.get("vel").copy())


@ALL_BUILDS
def test_sesph_permutation_spread_is_a_tenth_of_the_bars(double, kset):
    """the oracle on 5 permutations of the SESPH scene: density and forces of one stage (at the upload state and at the state four
    steps later), positions and velocities after one step, and in fp64 after 8 steps"""
    sc = S.sesph_scene(double, kset)
    stage, steps = (TOL_STAGE_F64, TOL_STEPS_F64) if double else (TOL_STAGE, TOL_STEPS)
    states = S.oracle_states(double, kset, 4)
    base = {w: _stage(sc, double, kset, *states[w]) for w in (0, 4)}
    base1 = _steps(sc, double, kset, *states[0], 1)
    base8 = _steps(sc, double, kset, *states[0], 8) if double else None
    d = dict(dens=0.0, forces=0.0, pos1=0.0, vel1=0.0, pos8=0.0, vel8=0.0)
    for seed in range(PERMUTATIONS):
        perm = np.random.default_rng(100 + seed).permutation(sc["n"])
        for w in (0, 4):
            dens, forces = _stage(sc, double, kset, states[w][0][perm], states[w][1][perm])
            d["dens"] = max(d["dens"], rel_err(dens, base[w][0]))
            d["forces"] = max(d["forces"], rel_err(forces, base[w][1]))
        p1, v1 = _steps(sc, double, kset, states[0][0][perm], states[0][1][perm], 1)
        d["pos1"], d["vel1"] = max(d["pos1"], rel_err(p1[:, :3], base1[0][:, :3])), max(d["vel1"], rel_err(v1[:, :3], base1[1][:, :3]))
        if double:
            p8, v8 = _steps(sc, double, kset, states[0][0][perm], states[0][1][perm], 8)
            d["pos8"], d["vel8"] = max(d["pos8"], rel_err(p8[:, :3], base8[0][:, :3])), max(d["vel8"], rel_err(v8[:, :3], base8[1][:, :3]))
    print("oracle permutation spread %s: %s" % (S.BUILD_IDS[S.BUILDS.index((double, kset))], {k: "%.2e" % v for k, v in d.items()}))
    assert max(d.values()) > 0, "no in-cell order in this scene: the wrong yardstick"
    for k in ("dens", "forces", "pos1", "vel1"):
        assert d[k] <= stage / 10, (k, d[k], stage)
    for k in ("pos8", "vel8"):
        assert d[k] <= steps / 10, (k, d[k], steps)


@pytest.mark.parametrize("walls", [False, True], ids=["nowall", "walls"])
@ALL_BUILDS
def test_iisph_permutation_spread_is_a_tenth_of_the_bars(double, kset, walls):
    """the by-slot IISPH oracle on 5 permutations of the IISPH scene, one step (the lockstep test restarts every step from
    identical bits): positions and velocities against the bars of that path"""
    p, pos, vel, bi, vbi = S.iisph_scene(double, kset, walls)
    sc = dict(p=p, bi=bi, vbi=vbi)
    tol_p, tol_v = (TOL_STEPS_F64, TOL_STEPS_F64) if double else (TOL_STEPS, 10 * TOL_STEPS)

    def run(pos, vel):
        o = _oracle(sc, double, kset, pos, vel, solver=IISPH, by_slot=True)
        o.step(1)
        return o.get("pos").copy(), o.get("vel").copy()

    bp, bv = run(pos, vel)
    tree = cKDTree(bp[:, :3])
    e_p = e_v = 0.0
    for seed in range(PERMUTATIONS):
        perm = np.random.default_rng(200 + seed).permutation(len(pos))
        gp, gv = run(pos[perm], vel[perm])
        dist, idx = tree.query(gp[:, :3])
        assert len(np.unique(idx)) == len(pos)
        e_p, e_v = max(e_p, rel_err(gp[:, :3], bp[idx, :3])), max(e_v, rel_err(gv[:, :3], bv[idx, :3]))
    print("oracle permutation spread iisph %s %s: pos %.2e vel %.2e" % (S.BUILD_IDS[S.BUILDS.index((double, kset))],
                                                                        "walls" if walls else "nowall", e_p, e_v))
    assert e_p <= tol_p / 10 and e_v <= tol_v / 10, (e_p, e_v)


@pytest.mark.parametrize("bug", ["one-cell-halo", "no-ghosts"])
@ALL_BUILDS
def test_modelled_slab_bugs_break_the_stage_bar(double, kset, bug):
    """the left of two slabs evaluated with the neighbour's particles beyond one cell removed (a halo of one cell where the density of
    the first halo cell needs two), or with all of them removed: the forces of the owned particles in the cell next to the cut differ
    from the full domain's by at least 100x the stage bar at the worse of the two states of the stage test, which asserts at both,
    and by at least 10x at each (fp32 Monaghan with a one-cell halo at the upload state: 1.0e-4, 50x the bar; four steps later 0.12).
    So the scene does have particles whose result depends on the outer halo cell."""
    sc = S.sesph_scene(double, kset)
    stage = TOL_STAGE_F64 if double else TOL_STAGE
    cut = sc["cuts"][2][1]
    worst = 0.0
    for which in (0, 4):
        pos, vel = S.oracle_states(double, kset, 4)[which]
        cx = slab.cell_of(pos[:, 0], sc["p"]["worldOrigin"][0][0], sc["p"]["cellSize"][0][0], sc["real"])
        keep = cx < (cut + 1 if bug == "one-cell-halo" else cut)
        near = np.flatnonzero(cx == cut - 1)
        assert len(near) > 10
        _, full = _stage(sc, double, kset, pos, vel)
        o = _oracle(sc, double, kset, pos[keep], vel[keep])
        o.step(1, stop=STOP_FORCES)
        ids = o.get("sortedVel")[:, 3].astype(np.int64)
        part = np.full((sc["n"], 4), np.nan, sc["real"])
        part[ids] = o.get("forces")
        e = rel_err(part[near], full[near])
        print("%s %s state %d: forces next to the cut off by %.2e (stage bar %.0e)" % (bug, S.BUILD_IDS[S.BUILDS.index((double, kset))],
                                                                                      which, e, stage))
        assert e >= 10 * stage, (which, e, stage)   # seen at either state ...
        worst = max(worst, e)
    assert worst >= 100 * stage, (worst, stage)     # ... and by 100x the bar by the stage test, which asserts at both


@pytest.mark.parametrize("kset", [1, 0], ids=["muller", "monaghan"])
def test_fp64_bars_tell_fp32_from_fp64_on_the_slab_scenes(kset):
    """the fp32 scenes, widened exactly, in the fp32 and the fp64 oracle, compared by id (a particle put one fp32 step from a cell
    face may sit in another cell once widened: the sort orders differ): one stage, one step and 8 steps of SESPH, one step of by-slot
    IISPH (paired by position).  Every difference is at least 100x the fp64 bar it would be held against."""
    sc = S.sesph_scene(False, kset)
    ip, ipos, ivel, _, _ = S.iisph_scene(False, kset, False)
    outs = []
    for double in (False, True):
        real = np.float64 if double else np.float32
        sd = dict(bi=sc["bi"].astype(real), vbi=sc["vbi"].astype(real))
        sd["p"] = S.grid_params(Oracle.default_params(SESPH, double, kset), double, kset, SESPH, sd["bi"], sd["vbi"])
        pos, vel = sc["pos"].astype(real), sc["vel"].astype(real)
        got = dict(zip(("dens", "forces"), _stage(sd, double, kset, pos, vel)))
        for k in (1, 8):
            got["pos%d" % k], got["vel%d" % k] = (a[:, :3] for a in _steps(sd, double, kset, pos, vel, k))
        oi = Oracle(Oracle.default_params(IISPH, double, kset), double, kset, IISPH, tait="double7", self_by_slot=True)
        oi.set_particles(ipos.astype(real), ivel.astype(real))
        oi.set_boundaries(None, None)
        oi.step(1)
        got["ipos1"], got["ivel1"] = oi.get("pos")[:, :3].copy(), oi.get("vel")[:, :3].copy()
        outs.append(got)
    a, b = outs
    dist, idx = cKDTree(b["ipos1"]).query(a["ipos1"])
    assert len(np.unique(idx)) == len(idx) and dist.max() < 1e-5
    b["ipos1"], b["ivel1"] = b["ipos1"][idx], b["ivel1"][idx]
    d = {k: rel_err(a[k], b[k]) for k in a}
    print({k: "%.2e" % v for k, v in d.items()})
    for k, e in d.items():
        bar = TOL_STEPS_F64 if k in ("pos8", "vel8", "ipos1", "ivel1") else TOL_STAGE_F64
        assert e >= 100 * bar, (k, e, bar)


def test_mean_density_is_formed_in_the_solvers_precision():
    """slab.mean_density, the exit test's rho_avg = (SReal)sum / N: a mean of 1001.00003 leaves the loop in fp32 (rounds to 1001) and
    stays in it in fp64, and the sum itself is rounded to SReal before the division as the reference's `rho_avg = (SReal)acc` does"""
    tot, cnt = 1001.00003 * 7, 7
    assert not (float(slab.mean_density(tot, cnt, np.float32)) - 1000.0) > 1.0
    assert (float(slab.mean_density(tot, cnt, np.float64)) - 1000.0) > 1.0
    assert type(slab.mean_density(tot, cnt, np.float32)) is np.float32 and type(slab.mean_density(tot, cnt, np.float64)) is np.float64
    big = 16777217.0   # 2^24 + 1 is not an fp32 number: the sum is rounded first
    assert slab.mean_density(big, 1, np.float32) == np.float32(16777216.0) and slab.mean_density(big, 1, np.float64) == big
