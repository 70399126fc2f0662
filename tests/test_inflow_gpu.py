"""Sources and sinks on the device (include/nereus_hip.h "sources and sinks"; DESIGN.md "Sources and sinks").  The oracle of every
stepping test is a TWIN context with the same history that never uses the feature: it receives the particles of the numpy model
(tests/inflow_model.py) through nrs_upload_particles(first = n), or the model's survivors through nrs_set_num_particles and an upload,
then both step, and the downloads and n must be byte-equal — positions against the model and the state transition at once.  The
scenes and schedules are those of tests/test_inflow_model_cpu.py, where the model alone shows that they are not vacuous.
"""
import numpy as np
import pytest

from nereus_amd import capi
from tests import inflow_model as im
from tests.common import compressed_dam_break, small_dam_break
from tests.test_inflow_model_cpu import DT, DT_TWO, FAUCET, LOCKSTEP_STEPS, S, sink_scene

pytestmark = pytest.mark.gpu

BUILDS = [(False, capi.MULLER), (False, capi.MONAGHAN), (True, capi.MULLER), (True, capi.MONAGHAN)]
BUILD_IDS = ["f32-muller", "f32-monaghan", "f64-muller", "f64-monaghan"]
# SESPH in the four builds; the other solvers in fp32 Mueller
CASES = [(capi.SESPH, d, k) for d, k in BUILDS] + [(s, False, capi.MULLER) for s in (capi.IISPH, capi.PCISPH, capi.PBF, capi.DFSPH)]
CASE_IDS = ["sesph-" + b for b in BUILD_IDS] + ["iisph", "pcisph", "pbf", "dfsph"]
E_INVALID, E_CAPACITY, E_STATE = -1, -3, -4


def refused(code, call):
    with pytest.raises(capi.NereusError) as e:
        call()
    assert ("error %d:" % code) in str(e.value), str(e.value)
    assert len(str(e.value).split(":", 1)[1].strip()) > 0


def same_state(s, t, what):
    """n and the downloads (positions, velocities, pressures) of two contexts, byte for byte"""
    assert s.n == t.n, (what, s.n, t.n)
    for name, a, b in zip(("pos", "vel", "pres"), s.download(pressure=True), t.download(pressure=True)):
        if a.tobytes() != b.tobytes():
            bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
            raise AssertionError("%s: %s differs in %d of %d rows, first %d: %r against %r" % (what, name, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]]))


def pair(solver, double, ks, scene=None, capacity=None, fluid=True, params=None):
    """two contexts on small_dam_break's tank with the same history: (context, twin, params as the contexts hold them, scene)"""
    p, sc = scene if scene is not None else small_dam_break((12, 10, 9), double=double, kernel_set=ks, solver=solver)
    if params is not None:
        p = params
    out = []
    for _ in range(2):
        s = capi.Solver(p, capacity or len(sc["pos"]), solver=solver, double=double, kernel_set=ks)
        if solver == capi.DFSPH:
            s.dfsph_configure(warm_start=False)  # (an upload restarts Kv at zero: the twin could not follow a warm start)
        if fluid:
            s.set_particles(sc["pos"], sc["vel"])
        s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
        out.append(s)
    return out[0], out[1], out[0].params, sc


# ---- 1. emit_block: into an empty context and into the dam break, then three steps ------------------------------------------------------------
@pytest.mark.parametrize("solver,double,ks", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("fluid", [False, True], ids=["empty", "dam"])
def test_emit_block(solver, double, ks, fluid):
    s, t, p, sc = pair(solver, double, ks, capacity=(1080 if fluid else 0) + 105 + 50, fluid=fluid)  # (room for one block, not for two)
    h = float(p["interactionRadius"][0])
    origin, spacing, dims, vel = (0.9, 0.1, 0.1), (0.8 * h, 0.85 * h, 0.9 * h), (7, 5, 3), (0.25, -0.5, 0.125)
    n0 = s.n
    assert s.emit_block(origin, spacing, dims, vel) == 105 and s.n == n0 + 105
    pos, v4 = im.block(origin, spacing, dims, vel, s.real)
    t.set_particles(pos, v4, first=n0)
    same_state(s, t, "after the block")
    assert s.download()[0][n0:].tobytes() == pos.tobytes()
    for k in range(3):
        s.step(1)
        t.step(1)
        same_state(s, t, "step %d" % k)
    # all or nothing
    before = s.download(pressure=True)
    refused(E_CAPACITY, lambda: s.emit_block(origin, spacing, dims, vel))
    assert s.n == n0 + 105 and all(a.tobytes() == b.tobytes() for a, b in zip(before, s.download(pressure=True)))
    s.close()
    t.close()


# ---- 2. an emitter fills an empty tank in lockstep with the model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,double,ks", CASES[:4] + CASES[-1:], ids=CASE_IDS[:4] + CASE_IDS[-1:])
def test_emitter_lockstep(solver, double, ks):
    p0, sc = small_dam_break((12, 10, 9), double=double, kernel_set=ks, solver=solver)
    p0 = p0.copy()
    p0["timestep"][0] = DT
    s, t, p, _ = pair(solver, double, ks, scene=(p0, sc), capacity=600, fluid=False)
    assert s.n == 0 and t.n == 0
    s.emitter_set(0, **FAUCET)
    m = im.Emitter(p, **FAUCET)
    emitting = 0
    for k in range(LOCKSTEP_STEPS):
        dt = DT_TWO if k == 0 else DT
        if k < 2:  # the first step takes a dt that yields two layers
            q = s.params.copy()
            q["timestep"][0] = dt
            s.set_params(q)
            t.set_params(q)
        pos, vel = m.step(float(s.params["timestep"][0]), 600 - t.n, s.real)
        if len(pos):
            t.set_particles(pos, vel, first=t.n)
            emitting += 1
        assert len(pos) == (42 if k == 0 else len(pos)) and len(pos) in (0, 21, 42)
        s.step(1)
        t.step(1)
        same_state(s, t, "step %d" % k)
    assert emitting >= 6 and s.n == m.emitted == 21 * (emitting + 1)
    em, emitted, dropped = s.emitter_get(0)
    assert (emitted, dropped) == (m.emitted, 0) and em["direction"] == [0.0, -1.0, 0.0] and em["spacing"] == S and em["enabled"]
    s.close()
    t.close()


# ---- 3. compaction shapes: N = 3 * 256 + 7 particles placed by index inside or outside one box ---------------------------------------------------
N_SHAPES = 3 * 256 + 7
PATTERNS = {
    "none": lambda i: np.zeros(len(i), bool),
    "all": lambda i: np.ones(len(i), bool),
    "first": lambda i: i == 0,
    "last": lambda i: i == N_SHAPES - 1,
    "alternating": lambda i: i % 2 == 1,
    "one_workgroup": lambda i: (i >= 256) & (i < 512),
}


@pytest.mark.parametrize("double,ks", BUILDS[::3], ids=BUILD_IDS[::3])
def test_compaction_shapes(double, ks):
    p, _ = small_dam_break((12, 10, 9), double=double, kernel_set=ks)
    real = np.float64 if double else np.float32
    idx = np.arange(N_SHAPES)
    rng = np.random.default_rng(3)
    box = [0.5, 0.5, 0.5, 1.0, 1.0, 1.0]
    s = capi.Solver(p, N_SHAPES, double=double, kernel_set=ks)
    s.sinks_set([box])
    total, culls = 0, 0
    cases = list(PATTERNS.items()) + [("non_finite", None)]
    for name, pat in cases:
        pos = np.ones((N_SHAPES, 4), real)
        pos[:, :3] = rng.uniform(0.0, 0.4, (N_SHAPES, 3))
        if pat is None:  # every non-finite kind, outside the box: NaN or an infinity in one coordinate, in all, and a NaN w that does not count
            pos[5, 0], pos[300, 1], pos[511, 2], pos[512, :3], pos[N_SHAPES - 1, 0], pos[7, 3] = np.nan, np.inf, -np.inf, np.nan, -np.inf, np.nan
            inside = np.zeros(N_SHAPES, bool)
        else:
            inside = pat(idx)
            pos[inside, :3] = rng.uniform(0.5, 0.99, (int(inside.sum()), 3))
        vel = rng.uniform(-1, 1, (N_SHAPES, 4)).astype(real)
        pres = rng.uniform(0, 1, N_SHAPES).astype(real)
        s.set_particles(pos, vel, pres)
        gone = im.caught(p, pos, real, boxes=[box])
        assert gone.sum() == (5 if pat is None else inside.sum())
        removed = s.cull()
        want = im.compact(gone, pos, vel, pres)
        got = s.download(pressure=True)
        assert removed == int(gone.sum()) and s.n == N_SHAPES - removed, (name, removed)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes(), name
        total += removed
        culls += 1
        assert s.sinks_count() == (total, culls)
    s.close()


# 1026 workgroups of 256: the one scanning workgroup takes 1024 totals per pass, so its second pass starts from a carry
N_CARRY = 1024 * 256 + 256 + 7
CARRY_PATTERNS = {
    "every_third": lambda i: i % 3 == 0,
    "all_but_last": lambda i: i != N_CARRY - 1,
    "workgroups_1023_1024": lambda i: (i >= 1023 * 256) & (i < 1025 * 256),  # the last of the first pass, the first of the second
}


@pytest.mark.parametrize("double,ks", BUILDS[::3], ids=BUILD_IDS[::3])
def test_compaction_scan_carry(double, ks):
    """test_compaction_shapes at a size whose workgroup totals need two passes of the scan; no step is taken"""
    p, _ = small_dam_break((12, 10, 9), double=double, kernel_set=ks)
    real = np.float64 if double else np.float32
    idx = np.arange(N_CARRY)
    rng = np.random.default_rng(5)
    box = [0.5, 0.5, 0.5, 1.0, 1.0, 1.0]
    s = capi.Solver(p, N_CARRY, double=double, kernel_set=ks)
    s.sinks_set([box])
    total, culls = 0, 0
    for name, pat in CARRY_PATTERNS.items():
        inside = pat(idx)
        pos = np.ones((N_CARRY, 4), real)
        pos[:, :3] = rng.uniform(0.0, 0.4, (N_CARRY, 3))
        pos[inside, :3] = rng.uniform(0.5, 0.99, (int(inside.sum()), 3))
        vel = rng.uniform(-1, 1, (N_CARRY, 4)).astype(real)
        pres = rng.uniform(0, 1, N_CARRY).astype(real)
        s.set_particles(pos, vel, pres)
        gone = im.caught(p, pos, real, boxes=[box])
        assert gone.sum() == inside.sum()
        removed = s.cull()
        want = im.compact(gone, pos, vel, pres)
        got = s.download(pressure=True)
        assert removed == int(gone.sum()) and s.n == N_CARRY - removed, (name, removed)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes(), name
        total += removed
        culls += 1
        assert s.sinks_count() == (total, culls)
    s.close()


def test_compaction_moves_dfsph_kv():
    """after two DFSPH steps with the warm start, Kv is compacted like the positions"""
    p, sc = small_dam_break((12, 10, 9), solver=capi.DFSPH)
    vel = sc["vel"].copy()
    vel[:, :3] = np.random.default_rng(11).uniform(-0.3, 0.3, (len(vel), 3))
    s = capi.Solver(p, len(sc["pos"]), solver=capi.DFSPH)
    s.set_particles(sc["pos"], vel)
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    s.step(2)
    kv = s.get("dfsphKappaV")
    pos, v4, pres = s.download(pressure=True)
    assert len(kv) == len(pos) and np.count_nonzero(kv) > len(kv) // 2
    box = [-1.0, -1.0, -1.0, float(np.median(pos[:, 0])), 3.0, 3.0]
    gone = im.caught(s.params, pos, s.real, boxes=[box])
    assert len(np.unique(np.nonzero(gone)[0] // 256)) >= 3 and 0.25 * len(pos) < gone.sum() < 0.75 * len(pos)
    s.sinks_set([box])
    assert s.cull() == gone.sum()
    for a, b in zip(s.download(pressure=True) + (s.get("dfsphKappaV"),), im.compact(gone, pos, v4, pres, kv)):
        assert a.tobytes() == b.tobytes()
    s.step(1)  # (and the context steps on)
    assert np.isfinite(s.download()[0]).all()
    s.close()


# ---- 4. sinks in a run ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("solver,double,ks", CASES, ids=CASE_IDS)
def test_sinks_in_a_run(solver, double, ks, interval):
    p, sc, pos, vel, box = sink_scene(double, ks, solver)
    out = []
    for _ in range(2):
        c = capi.Solver(p, len(pos), solver=solver, double=double, kernel_set=ks)
        if solver == capi.DFSPH:
            c.dfsph_configure(warm_start=False)
        c.set_particles(pos, vel)
        c.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
        out.append(c)
    s, t = out
    s.sinks_set([box], domain=True, interval=interval)
    removed, culls = 0, 0
    for k in range(1, 9):
        if im.cull_due(k, interval):
            tp, tv, tpres = t.download(pressure=True)
            gone = im.caught(t.params, tp, t.real, boxes=[box], domain_on=True)
            culls += 1
            if gone.any():
                removed += int(gone.sum())
                t.set_particles(*im.compact(gone, tp, tv, tpres))
        s.step(1)
        t.step(1)
        same_state(s, t, "step %d" % k)
        assert s.sinks_count() == (removed, culls)
    assert removed >= 12 * 2 * 9 + 1 and culls == 8 // interval and s.n == len(pos) - removed
    s.close()
    t.close()


# ---- 5. nothing caught: no side effects -------------------------------------------------------------------------------------------------------------
def test_nothing_caught_is_free_of_side_effects():
    p, sc = small_dam_break((40, 30, 30))  # above the threshold of the coherent re-sort
    out = []
    for _ in range(2):
        c = capi.Solver(p, len(sc["pos"]), solver=capi.SESPH)
        c.set_particles(sc["pos"], sc["vel"])
        c.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
        out.append(c)
    s, t = out
    s.sinks_set([[50.0, 50.0, 50.0, 51.0, 51.0, 51.0]], domain=True)
    s.emitter_set(3, enabled=False, **FAUCET)
    for k in range(10):
        s.step(1)
        t.step(1)
        same_state(s, t, "step %d" % k)
    assert s.resort_stats() == t.resort_stats() and s.resort_stats()[0] > 0
    assert s.sinks_count() == (0, 10) and s.emitter_get(3)[1:] == (0, 0)
    s.close()
    t.close()


# ---- 6. book-keeping ----------------------------------------------------------------------------------------------------------------------------------
def faucet_run(capacity, steps, **kw):
    p0, sc = small_dam_break((12, 10, 9))
    p0 = p0.copy()
    p0["timestep"][0] = DT
    s = capi.Solver(p0, capacity)
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    cfg = dict(FAUCET)
    cfg.update(kw)
    s.emitter_set(0, **cfg)
    s.step(steps)
    return s


def test_counts_at_a_capacity_that_cuts_the_third_layer():
    s = faucet_run(50, 16)
    assert s.n == 42 and s.emitter_get(0)[1:] == (42, 42)
    s.close()
    s = faucet_run(600, 16, max_particles=50)
    assert s.n == 42 and s.emitter_get(0)[1:] == (42, 42)
    s.close()


def test_disable_enable_and_remove_a_slot():
    s = faucet_run(600, 4)
    assert s.n == 21
    s.emitter_set(0, enabled=False, **FAUCET)
    assert s.emitter_get(0)[1:] == (0, 0)  # a set restarts the counts
    s.step(8)
    assert s.n == 21 and s.emitter_get(0)[1:] == (0, 0)
    s.emitter_set(0, **FAUCET)
    s.step(4)
    assert s.n == 42 and s.emitter_get(0)[1:] == (21, 0)
    s.emitter_set(0)
    em, emitted, dropped = s.emitter_get(0)
    assert (emitted, dropped) == (0, 0) and em["speed"] == 0.0 and not em["enabled"]
    s.step(8)
    assert s.n == 42
    # two slots emit in one step (the step sorts: the download is not in emission order)
    s.emitter_set(2, **dict(FAUCET, center=(0.8, 0.4, 0.23)))
    s.emitter_set(1, **dict(FAUCET, center=(0.6, 0.4, 0.23)))
    s.step(4)
    x = s.download()[0][:, 0]
    assert s.n == 84 and [int((np.abs(x - c) < 3 * S).sum()) for c in (0.4, 0.6, 0.8)] == [42, 21, 21]
    assert s.emitter_get(1)[1:] == (21, 0) and s.emitter_get(2)[1:] == (21, 0)
    s.close()


def test_sampler_follows_emission_and_removal():
    s, t, p, sc = pair(capi.SESPH, False, capi.MULLER, capacity=1080 + 105)
    h = float(p["interactionRadius"][0])
    q = np.ones((64, 4), np.float32)
    q[:, :3] = np.random.default_rng(2).uniform((0.85, 0.05, 0.05), (1.1, 0.3, 0.2), (64, 3))
    s.sample_points(q, capi.FIELD_DENSITY)
    s.sample_points(q, capi.FIELD_DENSITY)
    b0 = s.sample_builds()
    origin, spacing, dims = (0.9, 0.1, 0.1), 0.8 * h, (7, 5, 3)
    s.emit_block(origin, spacing, dims)
    s.sample_points(q, capi.FIELD_DENSITY)
    assert s.sample_builds() == b0 + 1
    t.set_particles(*im.block(origin, spacing, dims, (0, 0, 0), s.real), first=1080)
    t.sample_points(q, capi.FIELD_DENSITY)
    got, want = s.sample_result(capi.FIELD_DENSITY), t.sample_result(capi.FIELD_DENSITY)
    assert got.tobytes() == want.tobytes() and np.count_nonzero(got) > 16
    s.sinks_set([[0.85, 0.0, 0.0, 2.0, 2.0, 2.0]])
    assert s.cull() == 105
    s.sample_points(q, capi.FIELD_DENSITY)
    assert s.sample_builds() == b0 + 2
    assert s.cull() == 0
    s.sample_points(q, capi.FIELD_DENSITY)
    assert s.sample_builds() == b0 + 2  # nothing removed: nothing rebuilt
    s.close()
    t.close()


def test_two_runs_are_identical():
    def run():
        s = faucet_run(600, 0)
        s.sinks_set([[0.0, 0.0, 0.0, 2.0, 0.1, 1.0]], domain=True, interval=2)  # a slab over the floor: what arrives there goes
        s.step(60)
        out = s.download(pressure=True) + (s.n, s.sinks_count(), s.emitter_get(0)[1:])
        s.close()
        return out
    a, b = run(), run()
    assert a[3:] == b[3:] and a[3] > 0 and a[4][0] > 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))


def test_refusals_on_the_device():
    p, sc = small_dam_break((12, 10, 9))
    s = capi.Solver(p, len(sc["pos"]) + 10)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    box = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
    before = s.download(pressure=True)
    refused(E_INVALID, lambda: s.emitter_set(16, **FAUCET))
    refused(E_INVALID, lambda: s._chk(s.lib.nrs_emitter_get(s.h, 16, None, None, None)))
    for kw in (dict(center=(np.nan, 0, 0)), dict(direction=(0, 0, 0)), dict(speed=-1.0), dict(spacing=-1.0), dict(spacing=1e-7), dict(shape=2),
               dict(half_extent=np.inf), dict(speed=np.inf)):
        refused(E_INVALID, lambda: s.emitter_set(0, **dict(FAUCET, **kw)))
    assert s.emitter_get(0) == s.emitter_get(5) and s.emitter_get(0)[0]["speed"] == 0.0  # a refused call changes nothing
    refused(E_INVALID, lambda: s.sinks_set([box] * 17))
    refused(E_INVALID, lambda: s.sinks_set([box], nboxes=17))
    refused(E_INVALID, lambda: s.sinks_set([[0.0, 0.0, 0.0, 1.0, 0.0, 1.0]]))
    refused(E_INVALID, lambda: s.sinks_set([[0.0, 0.0, np.nan, 1.0, 1.0, 1.0]]))
    refused(E_INVALID, lambda: s.sinks_set([box], flags=2))
    refused(E_INVALID, lambda: s.sinks_set([box], reserved=1))
    refused(E_CAPACITY, lambda: s.emit_block((0, 0, 0), 0.1, (11, 1, 1)))
    refused(E_INVALID, lambda: s.emit_block((0, 0, 0), 0.0, (2, 1, 1)))
    refused(E_INVALID, lambda: s.emit_block((0, 0, 0), 0.1, (2, 1, 1), vel=(0, np.nan, 0)))
    refused(E_INVALID, lambda: s._chk(s.lib.nrs_emit_block(s.h, None, None, None)))
    assert s.cull() == 0 and s.sinks_count() == (0, 1) and s.n == len(sc["pos"])  # no sinks were stored
    # mid-update after a partial step
    s.step_partial(capi.STAGE_DENSITY)
    refused(E_STATE, lambda: s.emitter_set(0, **FAUCET))
    refused(E_STATE, lambda: s.sinks_set([box]))
    refused(E_STATE, lambda: s.cull())
    refused(E_STATE, lambda: s.emit_block((0, 0, 0), 0.1, (2, 1, 1)))
    s.set_particles(sc["pos"], sc["vel"])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, s.download(pressure=True)))
    # a context with sources or sinks cannot become a slab; a slab context refuses them
    s.sinks_set([box])
    refused(E_INVALID, lambda: s.slab_configure(0, 64, 8))
    s.sinks_set(None)
    s.emitter_set(7, enabled=False, **FAUCET)
    refused(E_INVALID, lambda: s.slab_configure(0, 64, 8))
    s.emitter_set(7)
    s.slab_configure(0, 64, 8)
    refused(E_INVALID, lambda: s.emitter_set(0, **FAUCET))
    refused(E_INVALID, lambda: s.sinks_set([box]))
    refused(E_INVALID, lambda: s.cull())
    refused(E_INVALID, lambda: s.emit_block((0, 0, 0), 0.1, (2, 1, 1)))
    s.close()
    # a host-driven IISPH step in progress: nrs_cull and nrs_emit_block wait for its end, the configuration calls do not
    p2, pos2, vel2, bi2, vbi2 = compressed_dam_break()
    t = capi.Solver(p2, len(pos2) + 10, solver=capi.IISPH)
    t.set_particles(pos2, vel2)
    t.set_boundaries(bi2, vbi2, update_grid=True)
    t.iisph_predict()
    refused(E_STATE, lambda: t.cull())
    refused(E_STATE, lambda: t.emit_block((0.5, 0.5, 0.2), 0.1, (2, 1, 1)))
    t.sinks_set([[50.0, 50.0, 50.0, 51.0, 51.0, 51.0]])
    t.iisph_iterate()
    t.iisph_finish()
    assert t.cull() == 0 and t.emit_block((0.5, 0.5, 0.2), 0.1, (2, 1, 1)) == 2
    t.close()


def test_host_driven_iisph_applies_sinks_at_predict():
    """nrs_iisph_predict culls and emits like nrs_step: the twin steps with nrs_step on the model's survivors"""
    p, pos, vel, bi, vbi = compressed_dam_break()
    out = []
    for _ in range(2):
        c = capi.Solver(p, len(pos), solver=capi.IISPH)
        c.set_particles(pos, vel)
        c.set_boundaries(bi, vbi, update_grid=True)
        out.append(c)
    s, t = out
    box = [-1.0, float(np.percentile(pos[:, 1], 80)), -1.0, 3.0, 3.0, 3.0]
    s.sinks_set([box])
    gone = im.caught(t.params, pos, t.real, boxes=[box])
    assert 0 < gone.sum() < len(pos)
    t.set_particles(*im.compact(gone, pos, vel))
    s.iisph_predict()
    assert s.n == t.n
    t.iisph_predict()
    for c in (s, t):
        c.iisph_iterate()
        c.iisph_iterate()
        c.iisph_finish()
    same_state(s, t, "after the host-driven step")
    s.close()
    t.close()
