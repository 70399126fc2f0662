"""The coherent re-sort (nrs_kernels_resort.h: k_reorder_merged; nrs_host_state.h: RESORT_MIN_PARTICLES = 32,768; nrs_host_plan.h:
plan_step) with every feature that rides on it: moving boundary bodies, Akinci surface tension and adhesion, the PBF extras, emitters
and sinks that change n, and the Monaghan and fp64 builds of every solver.

Every scene is the tank of small_dam_break((33, 32, 32)): 33,792 particles, 132 workgroups of 256, the smallest jittered tank above
the threshold (IISPH and DFSPH: compressed_dam_break's lattice of the same size in the same tank, so that their pressure solves have
work to do, tank(); the test whose sink takes two whole layers away: two layers taller, INFLOW_LATTICE).  The fluid gets the small
deterministic velocity field of the DFSPH tests (0.3 m/s: between 1 and 2 % of the particles change cell per step), because the resting tank yields next to no movers and a step without movers merges the stayers alone.

Every comparison is bit for bit; there is no tolerance in this file.  A test drives a default context and an NRS_FLAG_FULL_SORT
context (IISPH: | NRS_FLAG_NO_FUSION, as test_iisph_coherent_resort_equals_full_sort) identically, with fixed iteration counts, and
asserts
  - positions, velocities, pressures, hash, index, dens and the solver's carried arrays equal between the two after every checked step;
  - hash and index of the default context equal to tests/common.next_sorted_keys on the positions downloaded before the step: the
    numpy model of the order, which does not know about either sort path, so an error both paths share cannot hide;
  - at the end, on both contexts stopped behind the reorder (a finished step has reset the cell table): cellStart / cellEnd equal
    (check_cell_tables) and equal to the table of the model's keys, the sorted positions and velocities equal to the model's gather;
  - nrs_resort_stats of the default context: by the rule in the docstring of tests/test_call_sequences_gpu.py every full step behind a
    full step on the same arrays, grid and count takes the queued split and counts 1, so (steps on unchanged arrays - 1, 0), each test
    stating its number; (0, 0) on the full-sort context; NRS_STAT_MOVERS above 0 at least once (the mover merge ran) and below n / 4
    throughout (half the share at which a step falls back to the full sort).
Every test prints its nrs_resort_stats and its largest NRS_STAT_MOVERS.
"""
import numpy as np
import pytest

from nereus_amd import capi
from tests import inflow_model as im
from tests import track_model as tm
from tests.common import SOLVER_NAMES as NAMES, SOLVERS, check_cell_tables, compressed_dam_break, next_sorted_keys, plate_solver, small_dam_break
from tests.test_akinci_gpu import BETA, GAMMA
from tests.test_bodies_gpu import same as same_tables, state
from tests.test_inflow_gpu import BUILD_IDS, BUILDS
from tests.test_inflow_model_cpu import DT, DT_TWO, FAUCET
from tests.test_pbf_extras_gpu import DQ, EPS_V, K

pytestmark = pytest.mark.gpu

LATTICE = (33, 32, 32)
INFLOW_LATTICE = (33, 34, 32)   # the next lattice that stays above the threshold once its top two layers (2,112 particles) are caught: 35,904 -> 33,792
FULL = capi.FLAG_FULL_SORT
RED = (1.0, 0.0, 0.0, 1.0)
# what each solver carries from step to step, or leaves behind a step, besides the particle arrays
CARRIED = {capi.SESPH: (), capi.IISPH: ("P_l", "sumDij"), capi.PCISPH: ("P_l", "forcesP", "posPred"), capi.PBF: ("P_l", "forcesP", "posPred"),
           capi.DFSPH: ("dfsphAlpha", "P_l", "velAdv", "dfsphKappaV", "pres")}
_scenes = {}


def tank(solver=capi.SESPH, double=False, ks=capi.MULLER, speed=0.3, lattice=LATTICE):
    """(params, pos, vel, bi, vbi): the tank with the resting lattice, or for IISPH and DFSPH compressed_dam_break's; the velocity field on.
    compressed_dam_break's own spacing, 0.72 h, is 1.34 times the rest density with the Muller kernels: the column bursts, more than half
    of the particles change cell within three steps and the steps fall back to the full sort (seen on the device: nrs_resort_stats
    (6, 5) for DFSPH), which is not the path under test.  So the spacing is a mild one that still leaves the solves work to do
    (asserted: has_work): 0.80 h with the Muller kernels, where the particles next to the walls and the floor are above rest density
    (tests/test_dfsph_gpu.py squeezes its column to the same spacing for its re-sort test), 0.84 h with the Monaghan kernels."""
    key = (solver in (capi.IISPH, capi.DFSPH), double, ks, speed, lattice)
    if key not in _scenes:
        if key[0]:
            p, pos, vel, bi, vbi = compressed_dam_break(lattice, double=double, kernel_set=ks, ratio=0.80 if ks == capi.MULLER else 0.84)
        else:
            p, sc = small_dam_break(lattice, double=double, kernel_set=ks)
            pos, vel, bi, vbi = sc["pos"], sc["vel"], sc["bi"], sc["vbi"]
        k = np.arange(len(pos))
        vel = vel.copy()
        vel[:, 0] = speed * np.sin(k)
        vel[:, 1] = speed * np.cos(0.7 * k)
        _scenes[key] = (p, pos, vel, bi, vbi)
    return _scenes[key]


def full_sort_flags(solver):
    return FULL | (capi.FLAG_NO_FUSION if solver == capi.IISPH else 0)


def configure(s, solver, xsph=0.0):
    """the fixed iteration counts of tests/common.plate_solver"""
    if solver == capi.DFSPH:
        s.dfsph_configure(0.0, 3, 0.0, 3, 1)
    if solver == capi.PBF:
        s.pbf_configure(0.0, 3, 0.01, xsph)
    if solver in (capi.PCISPH, capi.IISPH):
        s.set_max_iterations(4)


def context(sc, solver, flags=0, double=False, ks=capi.MULLER, capacity=None, xsph=0.0, setup=None):
    p, pos, vel, bi, vbi = sc
    s = capi.Solver(p, capacity or len(pos), solver=solver, double=double, kernel_set=ks, flags=flags)
    s.set_particles(pos, vel)
    s.set_boundaries(bi, vbi, update_grid=True)
    configure(s, solver, xsph)
    if setup:
        setup(s)
    return s


def has_work(s):
    """IISPH, DFSPH: the pressure solve found something to do (positive pressures, positive K)"""
    if s.solver == capi.IISPH:
        return bool(s.download(pressure=True)[2].max() > 0)
    return s.solver != capi.DFSPH or bool(s.get("pres").max() > 0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def snapshot(s, extra=()):
    o = dict(zip(("pos", "vel", "pressure"), s.download(pressure=True)))
    for name in ("hash", "index", "dens") + CARRIED[s.solver] + tuple(extra):
        o[name] = s.get(name)
    return o


def same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        np.testing.assert_array_equal(bits(a[name]), bits(b[name]), err_msg="%s: %s" % (what, name))


def model_holds(s, want, what):
    """hash and index of the step just taken, byte for byte, against next_sorted_keys of the positions it started from"""
    for name, w in zip(("hash", "index"), want):
        got = s.get(name)
        assert got.dtype == w.dtype and got.tobytes() == w.tobytes(), "%s: %s differs from the order model in %d of %d slots" % (
            what, name, int((got != w).sum()) if got.shape == w.shape else -1, len(w))


class Movers:
    """NRS_STAT_MOVERS of the default context behind every call: the largest, and that it stays far from the fall-back share.  A step falls
    back to the full sort above RESORT_MAX_MOVER_PCT = 50 % movers (nrs_host_state.h: few_movers); that none did is the second number of
    nrs_resort_stats, asserted exactly, and the largest share seen stays below half of that bar, 25 %."""

    def __init__(self):
        self.seen = []

    def look(self, s):
        self.seen.append(s.get_stat(capi.STAT_MOVERS))

    def check(self, s, what, want_stats, share=True):
        got = s.resort_stats()
        print("%s: resort_stats %r, largest NRS_STAT_MOVERS %d of n = %d (per look: %r)" % (what, got, max(self.seen), s.n, [int(m) for m in self.seen]))
        assert got == want_stats, (what, got, want_stats)
        assert max(self.seen) > 0, (what, "no step had a mover: only the stayers-alone merge ran")
        assert not share or 4 * max(self.seen) < s.n, (what, self.seen)


def stopped_behind_the_reorder(d, f, what):
    """Both contexts stop behind the reorder of one more step (the default context's takes the queued split): the cell tables against each
    other and against the table of the model's keys, the sorted arrays against the model's gather.  Leaves both contexts mid-step."""
    pos, vel = d.download()
    keys, index = next_sorted_keys(d.params, pos, d.real)
    for s in (d, f):
        s.step_partial(capi.STAGE_REORDER)
    got = [(s.get("cellStart"), s.get("cellEnd")) for s in (d, f)]
    check_cell_tables(got[0][0], got[0][1], got[1][0], got[1][1])
    cells = int(np.prod(np.asarray(d.params["gridSize"]).reshape(-1)[:3].astype(np.int64)))
    assert len(got[0][0]) == cells
    start, end = np.full(cells, 0xFFFFFFFF, np.uint32), np.zeros(cells, np.uint32)
    uniq, first, count = np.unique(keys, return_index=True, return_counts=True)
    start[uniq], end[uniq] = first, first + count
    check_cell_tables(got[0][0], got[0][1], start, end)
    for s in (d, f):
        model_holds(s, (keys, index), what + ": stopped behind the reorder")
        np.testing.assert_array_equal(bits(s.get("sortedPos")), bits(pos[index]), err_msg=what + ": sortedPos")
        np.testing.assert_array_equal(bits(s.get("sortedVel")), bits(vel[index]), err_msg=what + ": sortedVel")


def three_plus_four_and_seven_singles(sc, solver, what, extra=(), xsph=0.0, setup=None):
    """Seven steps three ways: a default context as step(3), step(4); a default and a full-sort context as seven step(1) in lockstep, compared
    and held to the order model after each; the batched context compared after 3 and after 7.  Six steps find a queued split: (6, 0)."""
    n = len(sc[1])
    assert n >= 32768
    a, b = [context(sc, solver, 0, xsph=xsph, setup=setup) for _ in range(2)]
    c = context(sc, solver, full_sort_flags(solver), xsph=xsph, setup=setup)
    movers = Movers()
    a.step(3)
    for k in range(7):
        want = next_sorted_keys(b.params, b.download()[0], b.real)
        b.step(1)
        c.step(1)
        movers.look(b)
        model_holds(b, want, "%s step %d" % (what, k))
        same(snapshot(b, extra), snapshot(c, extra), "%s step %d, single steps against the full sort" % (what, k))
        if k == 2:
            same(snapshot(a, extra), snapshot(b, extra), what + ": step(3) against three single steps")
            a.step(4)
    same(snapshot(a, extra), snapshot(b, extra), what + ": step(3), step(4) against seven single steps")
    assert a.resort_stats() == (6, 0) and c.resort_stats() == (0, 0) and c.get_stat(capi.STAT_MOVERS) == -1.0, (a.resort_stats(), c.resort_stats())
    movers.check(b, what, (6, 0))
    assert has_work(b), what
    stopped_behind_the_reorder(b, c, what)
    assert b.resort_stats() == (7, 0) and c.resort_stats() == (0, 0)
    for s in (a, b, c):
        s.close()


# ---- 1. moving bodies ------------------------------------------------------------------------------------------------------------------------
_plates = {}


def tank_plate_scene():
    """tests/common.plate_scene at tank scale: the tank's fluid moved three cells from the wall x = 0 inside its boundary box (body 0), a
    plate of 32 x 32 boundary particles at fluid spacing, the size of the fluid's y-z face, one spacing in front of that wall (body 1),
    a single particle (body 2) and a bar of 7 (body 3), as far beyond the fluid's far face as plate_scene puts them."""
    if not _plates:
        p, pos, vel, bi, vbi = tank()
        h = float(p["interactionRadius"][0])
        d = h - 0.005
        pos = pos.copy()
        pos[:, 0] = (pos[:, 0].astype(np.float64) + 3.0 * h).astype(np.float32)
        far = float(pos[:, 0].max())

        def pts(a):
            o = np.ones((len(a), 4), np.float32)
            o[:, :3] = np.asarray(a, np.float64).astype(np.float32)
            return o

        jy, jz = np.meshgrid(np.arange(LATTICE[1]), np.arange(LATTICE[2]), indexing="ij")
        plate = pts(np.stack([np.full(jy.size, d), (jy.ravel() + 1) * d, (jz.ravel() + 1) * d], axis=1))
        dot = pts([[far + 0.27, 0.33, 0.21]])
        bar = pts(np.stack([far + 0.07 + np.arange(7) * d, np.full(7, 0.4), np.full(7, 0.23)], axis=1))
        parts = [bi, plate, dot, bar]
        walls = np.concatenate(parts)
        vols = np.concatenate([vbi] + [capi.boundary_volumes(a, h) for a in parts[1:]])
        body_of = np.concatenate([np.full(len(a), k, np.uint32) for k, a in enumerate(parts)])
        assert len(walls) % 256 != 0 and len(pos) >= 32768
        _plates["s"] = (p, pos, vel, walls, vols, body_of, parts)
    return _plates["s"]


@pytest.mark.parametrize("solver", SOLVERS, ids=[NAMES[k] for k in SOLVERS])
def test_moving_bodies(hip_lib, solver):
    """test_list_kernels_equal_reference_order_with_moving_walls (tests/test_bodies_gpu.py) where its full-sort leg is not vacuous: the
    default, the NRS_FLAG_NO_WALL_WORKGROUPS and the full-sort context equal each other in everything and the reference-order run in
    positions, velocities, the boundary tables, hash and index, while the boundary tables, nearBits and the wall workgroups' tile list
    are rebuilt every step under k_reorder_merged.  12 single steps, as that test takes, not 8: at PLATE_V the plate needs 10.2 steps
    from one spacing in front of the wall to come within h of fluid that stands three cells from it, and 9.8 to cross its second cell
    face, and both are asserted.  11 of the 12 steps find a queued split on the two contexts that re-sort: (11, 0)."""
    sc = tank_plate_scene()
    p = sc[0]
    steps = 12
    ref = plate_solver(sc, solver, reference_order=True)
    runs = [plate_solver(sc, solver), plate_solver(sc, solver, flags=capi.FLAG_NO_WALL_WORKGROUPS), plate_solver(sc, solver, flags=full_sort_flags(solver))]
    h, ox = float(p["interactionRadius"][0]), float(ref.params["worldOrigin"][0][0])
    cells, reach = set(), 0
    movers = [Movers(), Movers()]
    for step in range(steps):
        keys = next_sorted_keys(runs[0].params, runs[0].download()[0], np.float32)
        ref.step(1)
        want = state(ref, tables=True)
        want.update(hash=ref.get("hash"), index=ref.get("index"))
        px = ref.body_pose(1)[0][0]
        cells.add(int(np.floor((px - ox) / h)))
        reach += bool(px > float(want["pos"][:, 0].min()) - h)
        for s in runs:
            s.step(1)
        model_holds(runs[0], keys, "%s step %d" % (NAMES[solver], step))
        first = snapshot(runs[0])
        for k, s in enumerate(runs):
            got = state(s, tables=True)
            got.update(hash=s.get("hash"), index=s.get("index"))
            same_tables(got, want, "%s run %d step %d against the reference order:" % (NAMES[solver], k, step))
            if k:
                same(snapshot(s), first, "%s run %d step %d against the default context" % (NAMES[solver], k, step))
        for m, s in zip(movers, runs):
            m.look(s)
    assert len(cells) >= 3, cells     # the plate crossed two cell faces
    assert reach >= 2, reach          # ... into reach of fluid particles, for at least two of the steps
    assert runs[2].resort_stats() == (0, 0) and ref.resort_stats() == (0, 0)
    movers[0].check(runs[0], NAMES[solver] + " with moving bodies", (steps - 1, 0))
    movers[1].check(runs[1], NAMES[solver] + " with moving bodies, no wall workgroups", (steps - 1, 0))
    stopped_behind_the_reorder(runs[0], runs[2], NAMES[solver] + " with moving bodies")
    for s in runs + [ref]:
        s.close()


# ---- 2. Akinci surface tension and wall adhesion -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [capi.PCISPH, capi.PBF, capi.DFSPH], ids=["pcisph", "pbf", "dfsph"])
def test_akinci(hip_lib, solver):
    """gamma and beta of test_c3_one_dfsph_step_with_both_terms; the normals (valid from the first step on) among the compared arrays"""
    three_plus_four_and_seven_singles(tank(solver), solver, NAMES[solver] + " with Akinci", extra=("normals",), setup=lambda s: s.surface_akinci(GAMMA, BETA))


# ---- 3. PBF: tensile correction and vorticity confinement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("xsph", [0.0, 0.1])
def test_pbf_extras(hip_lib, xsph):
    """k_pbf_integrate emits the keys and the mover counts from its (xsph || vort) branch: with the confinement on, XSPH off and on;
    the vorticity (valid from the first step on) among the compared arrays"""

    def extras(s):
        s.pbf_set_tensile(K, DQ)
        s.pbf_set_vorticity(EPS_V)

    three_plus_four_and_seven_singles(tank(capi.PBF), capi.PBF, "pbf with s_corr and confinement, xsph %g" % xsph, extra=("vorticity",), xsph=xsph, setup=extras)


# ---- 4. emitters and sinks that change n -----------------------------------------------------------------------------------------------------------
def tracked(s):
    return s.track_result(capi.TRACK_ID), s.track_result(capi.TRACK_BIRTH), s.track_result(capi.TRACK_ATTRIBUTE)


def tracked_as_model(s, m, what):
    for name, got, want in zip(("ids", "births", "records"), tracked(s), (m.ids, m.birth, m.rec)):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, name)
    assert s.track_info() == (True, capi.TRACK_ATTR, m.next_id), (what, s.track_info(), m.next_id)


@pytest.mark.parametrize("solver", [capi.SESPH, capi.DFSPH], ids=["sesph", "dfsph"])
def test_emitters_and_sinks_change_n(hip_lib, solver):
    """Capacity n + 600.  The faucet of tests/test_inflow_model_cpu.py, moved next to the fluid's far face, emits a layer in steps 3 and 7
    (dt = DT: a quarter spacing per step) and two layers in step 9 (dt = DT_TWO; the last, because a step nine times as long kicks a
    resting fluid hard enough to throw particles into the sink for steps on end, which leaves no step with n unchanged: seen on the
    device).  A kill box over the top two lattice layers, as sink_run's, catches 2,112 particles before step 0, and NRS_SINK_DOMAIN is
    on; the lattice is two layers taller than the other tests', so that n stays above the threshold behind the cull.  The sinks and
    the emitters act at the top of a step, so a step whose own top caught or emitted something (particles_changed drops the queued
    split) hashes and sorts from scratch and counts nothing, and re-queues the split for the new n; every other step but the first
    takes the split and counts 1: steps 1, 2, 4, 5, 6 and 8 here, (6, 0) after the ten.  n follows inflow_model; the tracked ids,
    births and records follow track_model driven by the ORDER MODEL's index (not the device's), on every step: the top of a step that
    changes n is modelled too (survivors in order, then the layers).  SESPH: the ids hidden in vel.w are the witness that uses no
    index.  Then one emit_block and step(2): a scratch sort, then a merged step, (7, 0)."""
    p0, pos, vel, bi, vbi = tank(speed=0.1, lattice=INFLOW_LATTICE)   # (step 9 is nine times as long as the others: a third of the field keeps its movers few)
    p = p0.copy()
    p["timestep"][0] = DT
    n0, ny = len(pos), INFLOW_LATTICE[1]
    assert n0 >= 32768
    cap = n0 + 600
    if solver == capi.SESPH:
        vel = vel.copy()
        vel[:, 3] = np.arange(n0)
    d_lat = float(np.float32(p["interactionRadius"][0])) - 0.005   # the lattice spacing of scene.fluid_block
    box = [-1.0, (ny - 1.5) * d_lat, -1.0, 5.0, (ny + 2.0) * d_lat, 3.0]
    faucet = dict(FAUCET, center=(float(pos[:, 0].max()) + 0.1, 0.4, 0.23))   # its nearest sites stand 0.0375 from the fluid: inside h
    rec = np.ascontiguousarray(pos[:, [1, 2, 0, 3]])

    def setup(s):
        s.track_enable(capi.TRACK_ATTR)
        s.track_upload(capi.TRACK_ATTRIBUTE, rec)
        s.emitter_set(0, **faucet)
        s.track_emit_value(0, RED)
        s.sinks_set([box], domain=True)

    d, f = [context((p, pos, vel, bi, vbi), solver, flags, capacity=cap, setup=setup) for flags in (0, FULL)]
    real = d.real
    e = im.Emitter(d.params, **faucet)
    m = tm.State(n0, real)
    m.rec = rec.copy()
    m.values[0] = np.array(RED)
    movers = Movers()
    expect, quiet, changing = 0, 0, 0
    what = NAMES[solver] + " with a faucet and a sink"

    def compare(tag):
        assert d.n == f.n == m.n >= 32768, (tag, d.n, f.n, m.n)
        same(snapshot(d), snapshot(f), tag)
        for x, y in zip(tracked(d), tracked(f)):
            assert x.tobytes() == y.tobytes(), tag
        tracked_as_model(d, m, tag)
        if solver == capi.SESPH:
            old = m.ids < n0
            assert np.array_equal(d.download()[1][old, 3].astype(np.int64), m.ids[old].astype(np.int64)), tag
        assert d.resort_stats() == (expect, 0) and f.resort_stats() == (0, 0), (tag, d.resort_stats(), expect, f.resort_stats())

    def set_dt(dt):
        for s in (d, f):
            q = s.params.copy()
            q["timestep"][0] = dt
            s.set_params(q)

    for k in range(10):
        if k == 9:   # the last step takes a dt that yields two layers
            set_dt(DT_TWO)
        before = d.download()[0]
        gone = m.cull(d.params, before, boxes=[box], domain_on=True)
        layers, _ = e.step(float(d.params["timestep"][0]), cap - m.n, real)
        m.append(len(layers), slot=0)
        changed = bool(gone.any()) or len(layers) > 0
        want = next_sorted_keys(d.params, np.concatenate([before[~gone], layers]), real)
        d.step(1)
        f.step(1)
        movers.look(d)
        model_holds(d, want, "%s step %d (n %s)" % (what, k, "changed" if changed else "unchanged"))
        m.step(want[1])
        expect += int(k > 0 and not changed)
        quiet += int(k > 0 and not changed)
        changing += int(changed)
        compare("%s step %d" % (what, k))
        print("%s step %d: caught %d, emitted %d, n %d, resort_stats %r" % (what, k, int(gone.sum()), len(layers), d.n, d.resort_stats()))
    assert expect == 6 and quiet >= 2 and changing >= 2 and d.sinks_count()[0] == n0 + e.emitted - d.n >= 2 * 33 * 32 and e.emitted >= 4 * 21 and e.dropped == 0
    # one block between steps, the faucet and the sink off: the first of the two queued steps sorts from scratch, the second merges
    origin, spacing, dims = (float(pos[:, 0].max()) + 0.6, 0.1, 0.1), 0.04, (3, 2, 2)
    set_dt(DT)
    for s in (d, f):
        s.emitter_set(0, None)
        s.sinks_set(None)
        assert s.emit_block(origin, spacing, dims) == 12
    m.append(12)
    before = f.download()[0]
    assert before[-12:].tobytes() == im.block(origin, spacing, dims, (0.0, 0.0, 0.0), real)[0].tobytes()
    first = next_sorted_keys(f.params, before, real)
    f.step(1)                                    # (the full-sort context in single steps: it shows the state between the two)
    model_holds(f, first, what + ": the step behind the block")
    second = next_sorted_keys(f.params, f.download()[0], real)
    f.step(1)
    d.step(2)
    movers.look(d)
    model_holds(d, second, what + ": the second step behind the block")
    m.step(first[1])
    m.step(second[1])
    expect += 1
    compare(what + ": block, step(2)")
    movers.check(d, what, (expect, 0))
    d.close()
    f.close()


# ---- 5. the other builds ----------------------------------------------------------------------------------------------------------------------------
# test_coherent_resort_equals_full_sort and its siblings run SESPH in fp32 / fp64 Muller and the other four solvers in fp32 Muller: the rest
BUILD_CASES = [(s, dbl, ks) for s in SOLVERS for dbl, ks in BUILDS if not (ks == capi.MULLER and (s == capi.SESPH or not dbl))]
BUILD_CASE_IDS = ["%s-%s" % (NAMES[s], BUILD_IDS[BUILDS.index((dbl, ks))]) for s, dbl, ks in BUILD_CASES]


@pytest.mark.parametrize("solver,double,ks", BUILD_CASES, ids=BUILD_CASE_IDS)
def test_builds(hip_lib, solver, double, ks):
    """The shape of test_coherent_resort_equals_full_sort, steps (1, 2, 4), in the Monaghan and fp64 builds.  The default context takes
    each batch as one nrs_step call; the full-sort context takes its last step alone, which shows the positions that step starts from
    to the order model.  The Monaghan builds: outside SESPH plan_features().listKernels is false there, so the step runs the
    reference-order walks (k_walk_ref) without hit lists; plan_step() sets keys and resort all the same, the last launch of that chain
    emits the keys and the mover counts, and the split IS queued: (6, 0) like every other build, asserted first.  The one exception is
    IISPH with the Monaghan kernels, (6, 1): the split is queued there too, but that solver's first step leaves NaN in most positions, as
    the reference's does (the parity table: "IISPH | fp32 Monaghan ... NaN in ~75 % of densCorr / forcesP"), so the second
    step finds all but two particles in another cell and falls back to the full sort once; from then on nothing moves any more and
    the steps merge the stayers alone.  Equality, the order model (which converts non-finite cell coordinates as the device does) and
    the cell tables hold there as everywhere; the mover share and has_work say nothing about a state of NaNs and are not asked.  DFSPH with the Monaghan kernels
    is the other case without the 25 % bar: its solves stir the column at every spacing tried on the device (0.60 h to the resting
    0.89 h: between 39 % and 98 % movers by the seventh step, fall-backs below 0.80 h); at tank()'s 0.84 h the largest share is 44 %
    (14,819 of 33,792) and no step falls back, which the exact (6, 0) holds it to."""
    sc = tank(solver, double, ks)
    assert len(sc[1]) >= 32768
    d = context(sc, solver, 0, double, ks)
    f = context(sc, solver, full_sort_flags(solver), double, ks)
    what = "%s %s" % (NAMES[solver], BUILD_IDS[BUILDS.index((double, ks))])
    movers = Movers()
    done = 0
    nan = solver == capi.IISPH and ks == capi.MONAGHAN
    for k in (1, 2, 4):
        if k > 1:
            f.step(k - 1)
        want = next_sorted_keys(f.params, f.download()[0], f.real)
        f.step(1)
        d.step(k)
        done += k
        movers.look(d)
        assert d.resort_stats() == (done - 1, int(nan and done > 1)) and f.resort_stats() == (0, 0), (what, done, d.resort_stats(), f.resort_stats())
        model_holds(d, want, "%s after %d steps" % (what, done))
        same(snapshot(d), snapshot(f), "%s after %d steps" % (what, done))
    movers.check(d, what, (6, int(nan)), share=not nan and not (solver == capi.DFSPH and ks == capi.MONAGHAN))
    assert nan or has_work(d), what
    stopped_behind_the_reorder(d, f, what)
    d.close()
    f.close()
