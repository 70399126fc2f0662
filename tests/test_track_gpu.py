"""Particle identity and attributes on the device (include/nereus_hip.h "particle identity and attributes"; DESIGN.md "Particle identity
and attributes") against the numpy model of tests/track_model.py, byte for byte: ids, births and records through steps of every
solver, the coherent re-sort, emission, culls, uploads and count changes; nrs_track_locate; nrs_track_diffuse in the four builds; the
refusals.  Every scene is small_dam_break((12, 10, 9)) unless said otherwise: 1080 particles, four full workgroups plus 56 slots.
"""
import numpy as np
import pytest

from nereus_amd import capi
from tests import inflow_model as im
from tests import track_model as tm
from tests.common import compressed_dam_break, default_scene, small_dam_break
from tests.test_diffuse_gpu import dam_solver
from tests.test_inflow_gpu import BUILD_IDS, BUILDS, CASE_IDS, CASES, refused
from tests.test_inflow_model_cpu import DT, DT_TWO, FAUCET, sink_scene
from tests.test_track_model_cpu import KAPPA, record_for

pytestmark = pytest.mark.gpu

E_INVALID, E_CAPACITY, E_STATE = -1, -3, -4
ID, BIRTH, ATTRIBUTE, SLOT_OF = capi.TRACK_ID, capi.TRACK_BIRTH, capi.TRACK_ATTRIBUTE, capi.TRACK_SLOT_OF
RED, BLUE, GREY = (1.0, 0.0, 0.0, 1.0), (0.0, 0.25, 1.0, 0.5), (0.5, 0.5, 0.5, 1.0)


def dam(solver=capi.SESPH, double=False, ks=capi.MULLER, lattice=(12, 10, 9), extra=0, flags=0, scene=None):
    p, sc = scene if scene is not None else small_dam_break(lattice, double=double, kernel_set=ks, solver=solver)
    s = capi.Solver(p, len(sc["pos"]) + extra, solver=solver, double=double, kernel_set=ks, flags=flags)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    return s, sc


def tracked(s):
    return s.track_result(ID), s.track_result(BIRTH), (s.track_result(ATTRIBUTE) if s.track_info()[1] & capi.TRACK_ATTR else None)


def same_as_model(s, m, what):
    ids, birth, rec = tracked(s)
    assert ids.tobytes() == m.ids.tobytes(), (what, "ids", ids[:8], m.ids[:8])
    assert birth.tobytes() == m.birth.tobytes(), (what, "birth", birth[:8], m.birth[:8])
    if m.rec is not None:
        assert rec.dtype == m.rec.dtype and rec.tobytes() == m.rec.tobytes(), (what, "records")
    assert s.track_info() == (True, capi.TRACK_ATTR if m.attr else 0, m.next_id), (what, s.track_info(), m.next_id)


# ---- 1. tracking does not disturb the step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,double,ks", CASES, ids=CASE_IDS)
def test_tracking_does_not_disturb_the_step(solver, double, ks):
    s, _ = dam(solver, double, ks)
    t, _ = dam(solver, double, ks)
    s.track_enable(capi.TRACK_ATTR)
    s.set_profiling(True)
    t.set_profiling(True)
    for _ in range(6):
        s.step(1)
        t.step(1)
    for a, b in zip(s.download(pressure=True), t.download(pressure=True)):
        assert a.tobytes() == b.tobytes()
    ms, mt = s.stage_ms(), t.stage_ms()
    assert set(ms) == set(mt)
    for name in ms:
        assert ms[name][1] == mt[name][1] + (6 if name == "reorder" else 0), (name, ms[name], mt[name])
    assert t.track_info() == (False, 0, 0)
    s.close()
    t.close()


# ---- 2. ids follow the particles ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,double,ks", CASES, ids=CASE_IDS)
def test_ids_follow_the_particles(solver, double, ks):
    s, sc = dam(solver, double, ks)
    n = len(sc["pos"])
    witness = solver == capi.SESPH
    if witness:  # an id hidden in vel.w travels with the particle on SESPH: a witness that does not use the index
        vel = sc["vel"].copy()
        vel[:, 3] = np.arange(n)
        s.set_particles(sc["pos"], vel)
    s.track_enable(0)
    m = tm.State(n, s.real, attr=False)
    same_as_model(s, m, "enabled")
    for k in range(6):
        s.step(1)
        m.step(s.get("index"))
        same_as_model(s, m, "step %d" % k)
        if witness:
            assert np.array_equal(s.download()[1][:, 3].astype(np.int64), m.ids.astype(np.int64))
    assert sorted(m.ids.tolist()) == list(range(n)) and not m.birth.any()
    s.close()


# ---- 3. queued steps ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [capi.SESPH, capi.DFSPH], ids=["sesph", "dfsph"])
def test_queued_steps(solver):
    out = []
    for queued in (True, False):
        s, sc = dam(solver)
        s.track_enable(capi.TRACK_ATTR)
        s.track_upload(ATTRIBUTE, record_for(sc["pos"], s.real))
        if queued:
            s.step(7)
        else:
            for _ in range(7):
                s.step(1)
        out.append(tracked(s))
        s.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
    assert out[0][0].tolist() != list(range(len(out[0][0])))


# ---- 4. the coherent re-sort -----------------------------------------------------------------------------------------------------------------------
def test_coherent_resort():
    scene = small_dam_break((33, 32, 32))  # 33,792 particles: above the threshold of the coherent re-sort
    n = len(scene[1]["pos"])
    vel = scene[1]["vel"].copy()
    vel[:, 3] = np.arange(n)
    out = []
    for flags in (0, capi.FLAG_FULL_SORT):
        s, sc = dam(scene=scene, flags=flags)
        s.set_particles(sc["pos"], vel)
        s.track_enable(0)
        s.step(4)
        ids = s.track_result(ID)
        assert np.array_equal(s.download()[1][:, 3].astype(np.int64), ids.astype(np.int64))
        steps, fallbacks = s.resort_stats()
        assert flags or steps > fallbacks, (steps, fallbacks)  # merged steps on the default context
        out.append(ids)
        s.close()
    assert out[0].tobytes() == out[1].tobytes() and sorted(out[0].tolist()) == list(range(n))


# ---- 5. emit and cull --------------------------------------------------------------------------------------------------------------------------------
def faucet_run(solver, steps=12):
    """two emitters of different colour fill an empty tank; the model follows step by step; -> (context, model)"""
    p0, sc = small_dam_break((12, 10, 9), solver=solver)
    p0 = p0.copy()
    p0["timestep"][0] = DT
    s = capi.Solver(p0, 600, solver=solver)
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    s.track_enable(capi.TRACK_ATTR)
    m = tm.State(0, s.real)
    far = dict(FAUCET, center=(0.8, 0.4, 0.23))
    s.emitter_set(0, **FAUCET)
    s.emitter_set(2, **far)
    s.track_emit_value(0, RED)
    s.track_emit_value(2, BLUE)
    m.values[0], m.values[2] = np.array(RED), np.array(BLUE)
    e0, e2 = im.Emitter(s.params, **FAUCET), im.Emitter(s.params, **far)
    for k in range(steps):
        if k < 2:  # the first step takes a dt that yields two layers
            q = s.params.copy()
            q["timestep"][0] = DT_TWO if k == 0 else DT
            s.set_params(q)
        dt = float(s.params["timestep"][0])
        first = m.next_id
        a = m.emit(e0, dt, 600 - m.n, 0)
        b = m.emit(e2, dt, 600 - m.n, 2)
        if a + b:  # consecutive from next_id, layer-major, slots ascending; born at the step counter; the slot's colour
            assert m.ids[-(a + b):].tolist() == list(range(first, first + a + b)) and np.all(m.birth[-(a + b):] == k)
            assert np.all(m.rec[m.n - a - b:m.n - b] == np.array(RED, s.real)) and np.all(m.rec[m.n - b:] == np.array(BLUE, s.real))
        s.step(1)
        m.step(s.get("index"))
        same_as_model(s, m, "faucet step %d" % k)
    assert m.n == s.n == 2 * 21 * (2 + steps // 4) and len(set(m.birth.tolist())) >= 3
    return s, m


def sink_run(solver, steps=4):
    """the sink scene: a box over the top two lattice layers and the domain, culled before every step; -> (context, model)"""
    p, sc, pos, vel, box = sink_scene(solver=solver)
    s = capi.Solver(p, len(pos) + 64, solver=solver)
    s.set_particles(pos, vel)
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    s.track_enable(capi.TRACK_ATTR)
    rec = record_for(pos, s.real)
    s.track_upload(ATTRIBUTE, rec)
    m = tm.State(len(pos), s.real)
    m.rec = rec.copy()
    s.sinks_set([box], domain=True)
    removed = []
    for k in range(steps):
        before = tracked(s)
        gone = m.cull(s.params, s.download()[0], boxes=[box], domain_on=True)
        removed.append(int(gone.sum()))
        s.step(1)
        if not gone.any():  # a cull that catches nothing changes nothing: the step is the plain gather
            assert all(a.tobytes() == b[s.get("index")].tobytes() for a, b in zip(tracked(s), before))
        m.step(s.get("index"))
        same_as_model(s, m, "sink step %d" % k)
    assert removed[0] == 12 * 2 * 9 + 1 and 0 in removed[1:] and s.sinks_count()[0] == sum(removed)
    return s, m


@pytest.mark.parametrize("solver", [capi.SESPH, capi.DFSPH], ids=["sesph", "dfsph"])
def test_emit_and_cull(solver):
    s, m = faucet_run(solver)
    s.close()
    s, m = sink_run(solver)
    s.close()


# ---- 6. locate ------------------------------------------------------------------------------------------------------------------------------------------
def test_locate():
    s, m = sink_run(capi.SESPH)
    s.emit_block((0.9, 0.1, 0.1), 0.04, (3, 2, 2))  # ids 1081 .. 1092 behind the survivors
    m.append(12)
    same_as_model(s, m, "block")
    # the particles with the ten smallest ids go too (a kill box around each), so that a range can start before the smallest living id
    pos = s.download()[0]
    low = np.argsort(m.ids)[:10]
    boxes = [[float(x) - 1e-4, float(y) - 1e-4, float(z) - 1e-4, float(x) + 1e-4, float(y) + 1e-4, float(z) + 1e-4] for x, y, z in pos[low, :3]]
    s.sinks_set(boxes)
    gone = m.cull(s.params, pos, boxes=boxes)
    assert s.cull() == int(gone.sum()) >= 10 and gone[low].all()
    same_as_model(s, m, "lowest ids culled")
    living = int(m.ids.min())
    assert living >= 10
    seen_absent = seen_present = False
    for first, count in ((0, m.next_id + 50), (living - 3, 300), (600, 257), (m.next_id - 5, 40), (5, 0), (m.next_id + 10, 7)):
        got = s.track_locate(first, count)
        assert got.dtype == np.uint32 and got.tobytes() == tm.locate(m.ids, first, count).tobytes(), (first, count)
        here = got != capi.TRACK_NONE
        assert np.array_equal(m.ids[got[here]].astype(np.int64), first + np.nonzero(here)[0])
        seen_absent |= bool((~here).any())
        seen_present |= bool(here.any())
        assert s.track_device_ptr(SLOT_OF)[1] == 4 * count
    assert seen_absent and seen_present
    s.close()


# ---- 7. upload and count rules ---------------------------------------------------------------------------------------------------------------------------
def test_upload_and_count_rules():
    s, sc = dam(extra=300)
    n = len(sc["pos"])
    s.track_enable(capi.TRACK_ATTR)
    m = tm.State(n, s.real)
    s.track_emit_value(-1, GREY)
    m.values[-1] = np.array(GREY)
    for _ in range(2):
        s.step(1)
        m.step(s.get("index"))
    pos, vel = s.download()
    s.set_particles(pos[10:110], vel[10:110], first=10)          # overwrite: the same particles
    m.upload(10, 100)
    same_as_model(s, m, "overwrite")
    s.set_particles(pos[:40], vel[:40], first=n)                  # append
    m.upload(n, 40)
    same_as_model(s, m, "append")
    s.set_particles(pos[:8], vel[:8], first=n + 36)               # half old, half new
    m.upload(n + 36, 8)
    same_as_model(s, m, "straddle")
    assert m.n == s.n == n + 44 and m.ids[-44:].tolist() == list(range(n, n + 44)) and np.all(m.birth[-44:] == 2)
    assert np.all(m.rec[-44:] == np.array(GREY, s.real))
    s._chk(s.lib.nrs_set_num_particles(s.h, 500))                 # shrink
    m.set_n(500)
    same_as_model(s, m, "shrink")
    s._chk(s.lib.nrs_set_num_particles(s.h, 700))                 # grow: fresh ids, never reused
    m.set_n(700)
    same_as_model(s, m, "grow")
    assert m.ids[500:].tolist() == list(range(n + 44, n + 244))
    births = np.arange(700, dtype=np.uint32)[::-1].copy()
    s.track_upload(BIRTH, births[5:25], first=5)
    m.birth = m.birth.copy()
    m.birth[5:25] = births[5:25]
    up = np.array([7, 0xFFFFFFFD, 3000], np.uint32)
    s.track_upload(ID, up, first=3)
    m.upload_ids(up, first=3)
    same_as_model(s, m, "id upload")
    assert s.track_info()[2] == 0xFFFFFFFE
    before = tracked(s)
    refused(E_CAPACITY, lambda: s.emit_block((0.9, 0.1, 0.1), 0.04, (2, 1, 1)))
    refused(E_CAPACITY, lambda: s._chk(s.lib.nrs_set_num_particles(s.h, 702)))
    assert s.n == 700 and s.track_info()[2] == 0xFFFFFFFE and all(a.tobytes() == b.tobytes() for a, b in zip(before, tracked(s)))
    assert s.emit_block((0.9, 0.1, 0.1), 0.04, (1, 1, 1)) == 1   # the last id
    m.append(1)
    same_as_model(s, m, "last id")
    assert m.ids[-1] == 0xFFFFFFFE
    refused(E_CAPACITY, lambda: s.emit_block((0.9, 0.1, 0.1), 0.04, (1, 1, 1)))
    s.emitter_set(0, **FAUCET)                                     # a step whose emitter would pass the last id changes nothing
    q = s.params.copy()
    q["timestep"][0] = DT_TWO
    s.set_params(q)
    state = s.download(pressure=True)
    refused(E_CAPACITY, lambda: s.step(1))
    assert s.n == 701 and s.emitter_get(0)[1:] == (0, 0) and all(a.tobytes() == b.tobytes() for a, b in zip(state, s.download(pressure=True)))
    s.track_enable(0)                                              # renumbers
    assert s.track_info() == (True, 0, 701) and s.track_result(ID).tolist() == list(range(701))
    s.step(1)
    assert s.n == 701 + 42
    s.close()


# ---- 8. diffusion -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_diffusion_matches_the_model(double, ks):
    s = dam_solver(double, ks)
    p = s.params
    pos = s.download()[0]
    walls = s.get("bSorted")
    s.track_enable(capi.TRACK_ATTR)
    rec = record_for(pos, s.real)
    s.track_upload(ATTRIBUTE, rec)
    dt = 0.5 / tm.stability(p, pos, KAPPA, 1.0, ks, walls)
    builds = s.sample_builds()
    for k in range(5):
        step_dt = 0.0 if k == 4 else dt  # (the last call takes the context's timestep)
        s.track_diffuse(KAPPA, step_dt)
        want = tm.diffuse(p, pos, rec, KAPPA, step_dt or float(p["timestep"][0]), ks, walls)
        got = s.track_result(ATTRIBUTE)
        if got.tobytes() != want.tobytes():
            bad = np.nonzero((got != want).any(axis=1))[0]
            raise AssertionError("call %d: %d of %d records differ, first %d: device %r model %r" % (k, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]]))
        assert got[:, 3].tobytes() == rec[:, 3].tobytes() and np.count_nonzero(got[:, 0] != rec[:, 0]) > len(rec) // 2
        assert s.sample_builds() == builds + k + 1  # the sampler's grid, once per particle state
        s.step(1)
        rec = got[s.get("index")]
        pos = s.download()[0]
        assert s.track_result(ATTRIBUTE).tobytes() == rec.tobytes()
    s.close()


def test_diffusion_without_boundaries():
    p, pos, vel = default_scene()
    s = capi.Solver(p, len(pos))
    s.set_particles(pos, vel)
    s.step(2)
    pos = s.download()[0]
    s.track_enable(capi.TRACK_ATTR)
    rec = record_for(pos, s.real)
    s.track_upload(ATTRIBUTE, rec)
    dt = 0.5 / tm.stability(s.params, pos, KAPPA, 1.0)
    s.track_diffuse(KAPPA, dt)
    got = s.track_result(ATTRIBUTE)
    assert got.tobytes() == tm.diffuse(s.params, pos, rec, KAPPA, dt).tobytes() and got[:, 3].tobytes() == rec[:, 3].tobytes()
    s.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    s, sc = dam(extra=8)
    n = len(sc["pos"])
    k4 = (1.0, 1.0, 1.0, 1.0)
    ids = np.arange(4, dtype=np.uint32)
    calls = [lambda: s.track_result(ID), lambda: s.track_device_ptr(ID), lambda: s.track_upload(ID, ids), lambda: s.track_emit_value(0, RED),
             lambda: s.track_locate(0, 4), lambda: s.track_diffuse(k4)]
    for c in calls:   # before enable
        refused(E_STATE, c)
    assert s.track_info() == (False, 0, 0)
    s.track_disable()
    refused(E_INVALID, lambda: s.track_enable(2))
    refused(E_INVALID, lambda: s.track_enable(0x80000001))
    assert s.track_info() == (False, 0, 0)
    s.track_enable(0)  # no attribute record
    for c in (lambda: s.track_result(ATTRIBUTE), lambda: s.track_device_ptr(ATTRIBUTE), lambda: s.track_emit_value(-1, RED), lambda: s.track_diffuse(k4),
              lambda: s.track_upload(ATTRIBUTE, np.zeros((2, 4), np.float32))):
        refused(E_STATE, c)
    refused(E_STATE, lambda: s.track_result(SLOT_OF))  # no locate yet
    refused(E_INVALID, lambda: s.track_result(4))
    refused(E_INVALID, lambda: s.track_upload(SLOT_OF, ids))
    refused(E_INVALID, lambda: s.track_upload(ID, np.array([1, capi.TRACK_NONE], np.uint32)))
    refused(E_INVALID, lambda: s.track_upload(ID, ids, first=n - 3))
    refused(E_INVALID, lambda: s.track_upload(ID, ids, first=n + 1))
    refused(E_INVALID, lambda: s._chk(s.lib.nrs_track_upload(s.h, ID, None, 0, 4)))
    refused(E_INVALID, lambda: s.track_locate(0, (1 << 27) + 1))
    assert s.track_result(ID).tolist() == list(range(n)) and s.track_info() == (True, 0, n)  # a refused call changes nothing
    s.track_enable(capi.TRACK_ATTR)
    refused(E_INVALID, lambda: s.track_emit_value(16, RED))
    refused(E_INVALID, lambda: s.track_emit_value(-2, RED))
    refused(E_INVALID, lambda: s._chk(s.lib.nrs_track_emit_value(s.h, 0, None)))
    for bad in ((-1.0, 0, 0, 0), (0, np.nan, 0, 0), (0, 0, 0, np.inf)):
        refused(E_INVALID, lambda: s.track_diffuse(bad))
    refused(E_INVALID, lambda: s.track_diffuse(k4, -1e-3))
    refused(E_INVALID, lambda: s.track_diffuse(k4, np.nan))
    refused(E_INVALID, lambda: s._chk(s.lib.nrs_track_diffuse(s.h, None, 0.0)))
    refused(E_INVALID, lambda: s.slab_configure(0, 64, 8))  # a tracking context cannot become a slab
    # mid-update after a partial step: the tracked arrays of the last completed state stay, the calls that read them refuse
    s.step(1)
    held = tracked(s)
    s.step_partial(capi.STAGE_DENSITY)
    for c in (lambda: s.track_result(ID), lambda: s.track_device_ptr(BIRTH), lambda: s.track_locate(0, 4), lambda: s.track_diffuse(k4)):
        refused(E_STATE, c)
    pos, vel = sc["pos"], sc["vel"]
    s.set_particles(pos[:16], vel[:16], first=3)  # (abandons the partial step; the same particles)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(held, tracked(s)))
    # enable, disable and enable again: 0 .. n-1 once more, nothing before the second enable
    s.track_disable()
    assert s.track_info() == (False, 0, 0)
    refused(E_STATE, lambda: s.track_result(ID))
    s.track_enable(0)
    assert s.track_result(ID).tolist() == list(range(n)) and not s.track_result(BIRTH).any()
    s.close()
    # a slab context does not track
    t, _ = dam()
    t.slab_configure(0, 64, 8)
    refused(E_INVALID, lambda: t.track_enable(0))
    t.close()
    # a host-driven IISPH step in progress
    p2, pos2, vel2, bi2, vbi2 = compressed_dam_break()
    u = capi.Solver(p2, len(pos2), solver=capi.IISPH)
    u.set_particles(pos2, vel2)
    u.set_boundaries(bi2, vbi2, update_grid=True)
    u.track_enable(capi.TRACK_ATTR)
    u.iisph_predict()
    for c in (lambda: u.track_result(ID), lambda: u.track_device_ptr(ID), lambda: u.track_locate(0, 4), lambda: u.track_diffuse(k4),
              lambda: u.track_enable(0), lambda: u.track_upload(ID, ids)):
        refused(E_STATE, c)
    index = u.get("index")
    u.iisph_iterate()
    u.iisph_iterate()
    u.iisph_finish()
    assert u.track_result(ID).tobytes() == index.tobytes() and np.all(u.track_result(BIRTH) == 0)
    u.close()
