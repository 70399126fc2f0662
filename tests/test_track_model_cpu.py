"""The numpy model of particle tracking (tests/track_model.py) alone: the diffusion keeps a constant record and a channel with kappa = 0
bit for bit, conserves the sum of every channel within a derived bound, obeys the maximum principle at half the stability limit and is
not vacuous; the moves of ids through a step, an emission, a cull and a locate on hand cases; and the scenes the GPU tests use
(tests/test_track_gpu.py) are not vacuous.  No GPU.

The fluid state is small_dam_break((12, 10, 9)) with the random velocities of tests/test_diffuse_gpu.py's dam_solver after its three
steps, taken here by the CPU oracle (the device's state differs from it by rounding; the GPU tests use the device's own).

The conservation bound.  t_ij = (a_i - a_j) * w_ij and t_ji are exact negatives (w_ij == w_ji bit for bit), so in exact arithmetic the
sum over i of a particle's update is zero.  What is left is rounding: a particle's accumulator rounds once per neighbour (at most k_max
times, the product's own rounding being the same on both sides of a pair), the scaling by 2 dt kappa rho0 once and the final sum once:
k_max + 2 roundings of values no larger than max|a| while lambda_i <= 1.  With eps = 2 u that is (k_max + 2) eps max|a| per particle
with a factor two to spare, and N times that for the sum.
"""
import numpy as np
import pytest

from tests import inflow_model as im
from tests import pcisph_model as pm
from tests import track_model as tm
from tests.common import small_dam_break
from tests.oracle_lib import SESPH, Oracle
from tests.test_inflow_model_cpu import DT, DT_TWO, FAUCET, sink_scene

KAPPA = (1.0, 0.5, 0.25, 0.0)  # (the last channel is copied)
_state = {}


def record_for(pos, real):
    """a smooth function of position plus a step in x, per channel"""
    x, y, z = (pos[:, a].astype(np.float64) for a in range(3))
    stepx = (x > np.median(x)).astype(np.float64)
    rec = np.stack([np.sin(3.0 * x) + y + stepx, 2.0 * stepx - 1.0 + 0.3 * z, z * z + 0.5 * x, np.cos(5.0 * y) + stepx], axis=1)
    return rec.astype(real)


def dam_state(double=False, ks=pm.MULLER):
    """(params, pos, bsorted) of the dam break after three oracle steps"""
    key = (double, ks)
    if key not in _state:
        p, sc = small_dam_break((12, 10, 9), double=double, kernel_set=ks)
        vel = sc["vel"].copy()
        vel[:, :3] = np.random.default_rng(11).uniform(-0.3, 0.3, (len(vel), 3))
        o = Oracle(p, double=double, kernel_set=ks, solver=SESPH)
        o.set_particles(sc["pos"], vel)
        o.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
        o.step(3)
        walls = np.array(o.get("sbi")).reshape(-1, 4).copy()  # (what NRS_ARR_B_SORTED holds: the sorted boundary particles, V_b in w)
        walls[:, 3] = np.array(o.get("svbi")).reshape(-1)
        _state[key] = (o.params, np.array(o.get("pos")).reshape(-1, 4).copy(), walls)
    return _state[key]


def half_limit_dt(p, pos, walls):
    """dt for which stability() is 0.5 (lambda is linear in dt)"""
    return 0.5 / tm.stability(p, pos, KAPPA, 1.0, walls=walls)


def bound(n, kmax, rec, real):
    return n * (kmax + 2) * float(np.finfo(real).eps) * np.abs(rec.astype(np.float64)).max(axis=0)


def test_constant_record_and_zero_kappa_are_bit_identical():
    p, pos, walls = dam_state()
    dt = half_limit_dt(p, pos, walls)
    const = np.tile(np.array([1.5, -2.25, 1e-3, 7.0], np.float32), (len(pos), 1))
    assert tm.diffuse(p, pos, const, KAPPA, dt, walls=walls).tobytes() == const.tobytes()
    rec = record_for(pos, np.float32)
    out = tm.diffuse(p, pos, rec, KAPPA, dt, walls=walls)
    assert out[:, 3].tobytes() == rec[:, 3].tobytes()
    assert tm.diffuse(p, pos, rec, (0.0, 0.0, 0.0, 0.0), dt, walls=walls).tobytes() == rec.tobytes()


@pytest.mark.parametrize("double,ks", [(False, pm.MULLER), (True, pm.MONAGHAN)], ids=["f32-muller", "f64-monaghan"])
def test_conservation_and_not_vacuous(double, ks):
    p, pos, walls = dam_state(double, ks)
    real = pm.real_of(p)
    rec = record_for(pos, real)
    dt = 0.5 / tm.stability(p, pos, KAPPA, 1.0, ks, walls)
    assert tm.stability(p, pos, KAPPA, dt, ks, walls) == pytest.approx(0.5, rel=1e-12)
    info = {}
    out = tm.diffuse(p, pos, rec, KAPPA, dt, ks, walls, info=info)
    n = len(pos)
    drift = np.abs(out.astype(np.float64).sum(axis=0) - rec.astype(np.float64).sum(axis=0))
    b = bound(n, info["kmax"], rec, real)
    print("drift", drift, "bound", b, "kmax", info["kmax"])
    assert info["kmax"] >= 4 and np.all(drift <= b)
    for c in range(3):  # more than half of the particles change value in the first step
        assert np.count_nonzero(out[:, c] != rec[:, c]) > n // 2, c
    # without the walls the densities differ, the sum is conserved all the same
    out2 = tm.diffuse(p, pos, rec, KAPPA, dt, ks, None, info=info)
    assert np.all(np.abs(out2.astype(np.float64).sum(axis=0) - rec.astype(np.float64).sum(axis=0)) <= bound(n, info["kmax"], rec, real))


def test_maximum_principle_at_half_the_limit():
    p, pos, walls = dam_state()
    rec = record_for(pos, np.float32)
    dt = half_limit_dt(p, pos, walls)
    info = {}
    tm.diffuse(p, pos, rec, KAPPA, dt, walls=walls, info=info)
    b = bound(len(pos), info["kmax"], rec, np.float32)
    lo, hi = rec.astype(np.float64).min(axis=0) - b, rec.astype(np.float64).max(axis=0) + b
    a = rec
    spread0 = a.astype(np.float64).std(axis=0)
    for _ in range(20):
        a = tm.diffuse(p, pos, a, KAPPA, dt, walls=walls)
        assert np.all(a.astype(np.float64) >= lo) and np.all(a.astype(np.float64) <= hi)
    assert np.all(a.astype(np.float64).std(axis=0)[:3] < spread0[:3])  # (and it does smooth)


def test_pair_weights_are_symmetric():
    p, pos, walls = dam_state()
    order, i, j, w = tm.weights(p, pos, walls=walls)
    fwd = dict(zip(zip(i.tolist(), j.tolist()), w.tolist()))
    assert len(fwd) == len(w) and all(fwd[(b, a)] == v for (a, b), v in fwd.items())
    assert np.all(w <= 0)  # (d . grad W <= 0: every neighbour pulls towards its value)


# ---- ids -----------------------------------------------------------------------------------------------------------------------------------------
def test_step_emit_cull_and_locate_on_hand_cases():
    s = tm.State(5, attr=True)
    s.rec[:] = np.arange(20).reshape(5, 4)
    s.step([3, 0, 4, 1, 2])
    assert s.ids.tolist() == [3, 0, 4, 1, 2] and s.rec[:, 0].tolist() == [12, 0, 16, 4, 8] and s.steps == 1
    s.values[-1] = np.array([1.0, 2.0, 3.0, 4.0])
    s.append(2)
    assert s.ids.tolist() == [3, 0, 4, 1, 2, 5, 6] and s.birth.tolist() == [0] * 5 + [1, 1] and s.rec[6].tolist() == [1, 2, 3, 4] and s.next_id == 7
    assert tm.locate(s.ids, 2, 4).tolist() == [4, 0, 2, 5]
    assert tm.locate(s.ids, 6, 3).tolist() == [6, tm.NONE, tm.NONE] and len(tm.locate(s.ids, 0, 0)) == 0
    p = small_dam_break()[0]
    pos = np.zeros((7, 4), np.float32)
    pos[[1, 5], 0] = 0.75
    gone = s.cull(p, pos, boxes=[[0.5, -1, -1, 1, 1, 1]])
    assert gone.tolist() == [False, True, False, False, False, True, False] and s.ids.tolist() == [3, 4, 1, 2, 6]
    s.upload(3, 4)   # slots 3 and 4 are the same particles, 5 and 6 are new
    assert s.ids.tolist() == [3, 4, 1, 2, 6, 7, 8] and s.next_id == 9
    s.set_n(2)
    s.set_n(4)
    assert s.ids.tolist() == [3, 4, 9, 10]
    s.upload_ids([100, 0xFFFFFFFD], first=1)
    assert s.ids.tolist() == [3, 100, 0xFFFFFFFD, 10] and s.next_id == 0xFFFFFFFE
    s.append(1)      # the last id
    with pytest.raises(tm.Exhausted):
        s.append(1)
    assert s.n == 5 and s.next_id == 0xFFFFFFFF and tm.birth_of(1 << 40) == 0xFFFFFFFF


def test_emitted_ids_follow_the_schedule():
    p = small_dam_break()[0]
    e = im.Emitter(p, **FAUCET)
    s = tm.State(0)
    counts = [s.emit(e, DT_TWO if k == 0 else DT, 600 - s.n, 0) for k in range(8)]
    assert counts == [42, 0, 0, 21, 0, 0, 0, 21] and s.ids.tolist() == list(range(84)) and s.next_id == 84
    assert s.birth.tolist() == [0] * 42 + [0] * 21 + [0] * 21  # (the model's step counter only moves with step())


def test_cull_scene_is_not_vacuous():
    """the sink scene of the GPU test: the cull removes between 10 % and 90 % of the particles and splits a 256-slot workgroup"""
    for double in (False, True):
        real = np.float64 if double else np.float32
        p, sc, pos, vel, box = sink_scene(double)
        gone = im.caught(p, pos, real, boxes=[box]) | im.caught(p, pos, real, domain_on=True)
        assert 0.1 * len(pos) < gone.sum() < 0.9 * len(pos)
        groups = np.arange(len(pos)) // 256
        assert any(0 < gone[groups == g].sum() < (groups == g).sum() for g in np.unique(groups))
