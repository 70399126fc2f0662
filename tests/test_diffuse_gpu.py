"""The diffuse particles on the device (include/nereus_hip.h "diffuse particles"; DESIGN.md "Diffuse particles") against the numpy model
of tests/diffuse_model.py, byte for byte, in the four builds: normals, potentials, births, kinds, positions, velocities, lifetimes,
counts and `dropped`.  The settings are those of tests/test_diffuse_model_cpu.py, where the model alone shows that they produce every
kind, hit the per-particle cap and overflow; the lockstep test asserts the same of its own run.
"""
import numpy as np
import pytest

from nereus_amd import capi
from tests import diffuse_model as dm
from tests.common import small_dam_break
from tests.test_diffuse_model_cpu import SETTINGS, STEPS

pytestmark = pytest.mark.gpu

BUILDS = [(False, capi.MULLER), (False, capi.MONAGHAN), (True, capi.MULLER), (True, capi.MONAGHAN)]
BUILD_IDS = ["f32-muller", "f32-monaghan", "f64-muller", "f64-monaghan"]
E_INVALID, E_STATE = -1, -4
POS, VEL, KIND, POT, BIRTHS, NORMALS = (capi.DIFFUSE_POS, capi.DIFFUSE_VEL, capi.DIFFUSE_KIND, capi.DIFFUSE_POTENTIALS, capi.DIFFUSE_BIRTHS,
                                        capi.DIFFUSE_NORMALS)
CAP_SMALL = 4204  # half the total of the model's unbounded run in test_diffuse_model_cpu.py (8409)


def refused(code, call):
    with pytest.raises(capi.NereusError) as e:
        call()
    assert ("error %d:" % code) in str(e.value), str(e.value)
    assert len(str(e.value).split(":", 1)[1].strip()) > 0


def dam_solver(double, ks, solver=capi.SESPH, moving=True, steps=3):
    """a context of its own on small_dam_break((12, 10, 9)): with the random velocities and the three steps of the sampler tests' dam
    state, or (moving False) at rest and unstepped"""
    p, sc = small_dam_break((12, 10, 9), double=double, kernel_set=ks, solver=solver)
    vel = sc["vel"].copy()
    if moving:
        vel[:, :3] = np.random.default_rng(11).uniform(-0.3, 0.3, (len(vel), 3))
    else:
        vel[:] = 0
    s = capi.Solver(p, len(sc["pos"]), solver=solver, double=double, kernel_set=ks)
    s.set_particles(sc["pos"], vel)
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    if moving and steps:
        s.step(steps)
    return s


def device_set(s):
    return s.diffuse_result(POS), s.diffuse_result(VEL), s.diffuse_result(KIND)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
        raise AssertionError("%s: %d of %d rows differ, first %d: device %r model %r" % (what, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]]))


def check_step(s, r, what, cap=None, dropped=None):
    """the device's state after a diffuse step against the model's result r of the same step"""
    keep = r["total"] if cap is None else min(cap, r["total"])
    same(s.diffuse_result(NORMALS), r["normals"], what + " normals")
    same(s.diffuse_result(POT), r["potentials"], what + " potentials")
    same(s.diffuse_result(BIRTHS), r["births"], what + " births")
    pos, vel, kind = device_set(s)
    same(kind, r["kind"][:keep], what + " kinds")
    same(pos, r["pos"][:keep], what + " positions and lifetimes")
    same(vel, r["vel"][:keep], what + " velocities")
    alive, by_kind, dr = s.diffuse_count()
    assert alive == keep and by_kind == [int((r["kind"][:keep] == k).sum()) for k in range(3)], (what, alive, by_kind)
    if dropped is not None:
        assert dr == dropped, (what, dr, dropped)
    return pos, vel


# ---- 1. lockstep with the model: ten diffuse steps, one nrs_step between them ----------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_lockstep_with_model(double, ks):
    s = dam_solver(double, ks)
    cfg = dm.config(capacity=1 << 15, **SETTINGS)
    s.diffuse_configure(**cfg)
    dpos, dvel = np.zeros((0, 4), s.real), np.zeros((0, 4), s.real)
    seen, capped, died = np.zeros(3, np.int64), False, False
    for k in range(STEPS):
        pos, vel = s.download()
        s.diffuse_step()
        r = dm.step(s.params, cfg, pos, vel, dpos, dvel, k, 0.0, ks)
        died |= r["survivors"] < len(dpos)
        dpos, dvel = check_step(s, r, "step %d" % k, dropped=0)
        seen = np.maximum(seen, r["by_kind"])
        capped |= bool((r["births"] == cfg["max_per_particle"]).any())
        s.step(1)
    print("lockstep %s: largest count per kind %s, alive %d" % (BUILD_IDS[BUILDS.index((double, ks))], seen, len(dpos)))
    assert seen.min() >= 50 and capped and died, (seen, capped, died)  # (not vacuous: every kind, the cap, deaths)
    s.close()


# ---- 2. kinds by upload ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_kinds_by_upload(double, ks):
    s = dam_solver(double, ks, moving=False)
    real, p = s.real, s.params
    fpos, fvel = s.download()
    dt = real(p["timestep"][0])
    h = float(p["interactionRadius"][0])
    # k_drag = 1, no buoyancy: a bubble takes the Shepard velocity; the fluid rests, so nothing is born
    cfg = dm.config(capacity=16, seed=1, spray_below=3, bubble_above=6, k_drag=1.0, k_buoyancy=0.0)
    order = dm.sorted_order(p, fpos, real)
    sx, sv = fpos[order, :3], fvel[order, :3]
    cand = np.random.default_rng(6).uniform(fpos[:, :3].min(0), fpos[:, :3].max(0), (400, 3)).astype(real)
    _, n = dm.shepard(p, sx, sv, cand, ks)
    foam_at, bubble_at = cand[np.nonzero((n >= 3) & (n <= 6))[0][0]], cand[np.nonzero(n >= 8)[0][0]]
    wo = np.asarray(p["worldOrigin"]).reshape(-1)[:3].astype(real)
    hi = wo + np.asarray(p["gridSize"]).reshape(-1)[:3].astype(real) * np.asarray(p["cellSize"]).reshape(-1)[:3].astype(real)
    far = (hi - real(0.1)).astype(real)                      # inside the grid box, far from the fluid
    far[0] = hi[0] - real(0.8)
    edge = np.array((float(hi[0]) - 1e-4, float(far[1]), float(far[2])), real)
    assert not dm.shepard(p, sx, sv, np.stack((far, edge)), ks)[1].any()
    up = np.zeros((4, 4), real)
    uv = np.zeros((4, 4), real)
    up[0, :3], up[0, 3], uv[0, :3] = far, 1.0, (0.25, 0.5, -0.125)        # spray, far from the fluid
    up[1, :3], up[1, 3], uv[1, :3] = bubble_at, 1.0, (0.3, -0.2, 0.1)     # a bubble inside the resting block
    up[2, :3], up[2, 3], uv[2, :3] = foam_at, real(3.5) * dt, (1.0, 1.0, 1.0)  # foam with 3.5 steps to live
    up[3, :3], up[3, 3], uv[3, :3] = edge, 1.0, (1.0, 0.0, 0.0)           # crosses the high x face in the first step
    s.diffuse_configure(**cfg)
    s.diffuse_upload(up, uv)
    assert s.diffuse_count() == (4, [4, 0, 0], 0)
    same(s.diffuse_result(POS), up, "uploaded positions")
    dpos, dvel = up, uv
    g = np.asarray(p["gravity"]).reshape(-1)[:3].astype(real)
    bx, bv = far.copy(), uv[0, :3].copy()
    alive = []
    for k in range(5):
        s.diffuse_step()
        r = dm.step(p, cfg, fpos, fvel, dpos, dvel, k, 0.0, ks)
        dpos, dvel = check_step(s, r, "upload step %d" % k, dropped=0)
        assert not r["births"].any()
        alive.append(len(dpos))
        bv = bv + dt * g   # the closed-form ballistic state in the model's rounding order
        bx = bx + dt * bv
        assert dpos[0, :3].tobytes() == bx.tobytes() and dvel[0, :3].tobytes() == bv.tobytes() and dpos[0, 3] == 1.0
        if k == 0:
            assert list(r["kind"]) == [0, 2, 1] and not dvel[1].any() and not dvel[2].any()  # bubble and foam took vt = 0 exactly
            assert dpos[1].tobytes() == up[1].tobytes()
        if k < 3:
            assert dpos[2, 3] == up[2, 3] - real(k + 1) * dt or abs(float(dpos[2, 3]) - (3.5 - k - 1) * float(dt)) < 1e-6 * float(dt)
    assert alive == [3, 3, 3, 2, 2]  # the crosser is gone after the first step, the foam at the step its lifetime passes 0
    s.close()


# ---- 3. compaction across workgroups ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_compaction_across_workgroups(double, ks):
    s = dam_solver(double, ks, moving=False)
    real, p = s.real, s.params
    fpos, fvel = s.download()
    dt = real(p["timestep"][0])
    m = 3 * 256 + 7
    cfg = dm.config(capacity=m + 5, seed=3, spray_below=0, bubble_above=10 ** 6)  # everything is foam
    up = np.zeros((m, 4), real)
    up[:, :3] = np.random.default_rng(7).uniform(fpos[:, :3].min(0), fpos[:, :3].max(0), (m, 3)).astype(real)
    uv = np.zeros((m, 4), real)
    uv[:, :3] = 0.5
    s.diffuse_configure(**cfg)
    for name, life in (("alternating", np.where(np.arange(m) % 2 == 0, dt / real(2), real(10))), ("none", np.full(m, dt / real(2))),
                       ("all", np.full(m, real(10)))):
        up[:, 3] = life
        s.diffuse_upload(up, uv)
        s.diffuse_step()
        pos, vel, kind = device_set(s)
        long_lived = np.nonzero(life > dt)[0]
        assert len(pos) == len(long_lived) and np.all(kind == 1), name
        # the fluid rests: foam stays where it is and takes velocity 0; the survivors are the long-lived ones in upload order
        same(pos[:, :3], up[long_lived, :3], name + " positions")
        same(pos[:, 3], (up[long_lived, 3] - dt).astype(real), name + " lifetimes")
        assert not vel.any()
        r = dm.step(p, cfg, fpos, fvel, up, uv, 0, 0.0, ks)
        same(pos, r["pos"], name + " model")
        assert s.diffuse_count() == (len(long_lived), [0, len(long_lived), 0], 0)
    s.close()


# ---- 4. capacity: the births that fit are the first ones ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_capacity_keeps_the_first_births(double, ks):
    s = dam_solver(double, ks)
    cfg = dm.config(capacity=CAP_SMALL, **SETTINGS)
    s.diffuse_configure(**cfg)
    fpos, fvel = s.download()
    dpos, dvel = np.zeros((0, 4), s.real), np.zeros((0, 4), s.real)
    dropped = 0
    for k in range(8):
        s.diffuse_step()
        r = dm.step(s.params, cfg, fpos, fvel, dpos, dvel, k, 0.0, ks, capacity=1 << 30)  # the model's unbounded step from the device's state
        dropped += max(0, r["total"] - CAP_SMALL)
        dpos, dvel = check_step(s, r, "capacity step %d" % k, cap=CAP_SMALL, dropped=dropped)
        assert len(dpos) <= CAP_SMALL
    assert dropped > 0 and len(dpos) == CAP_SMALL
    # configure again with the same capacity: the set stays, `dropped` and the step counter restart
    s.diffuse_configure(**cfg)
    assert s.diffuse_count()[0] == CAP_SMALL and s.diffuse_count()[2] == 0
    same(s.diffuse_result(POS), dpos, "kept over configure")
    # another capacity: the set goes
    s.diffuse_configure(**dm.config(capacity=100, **SETTINGS))
    assert s.diffuse_count() == (0, [0, 0, 0], 0)
    s.diffuse_step()
    assert s.diffuse_count()[0] == 100 and s.diffuse_count()[2] > 0
    s.close()


# ---- 5. read-only ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_diffuse_steps_change_no_step(double, ks):
    for solver in (capi.SESPH, capi.IISPH, capi.DFSPH):
        a, b = dam_solver(double, ks, solver, steps=0), dam_solver(double, ks, solver, steps=0)
        a.diffuse_configure(**dm.config(capacity=1 << 14, **SETTINGS))
        for k in range(6):
            a.step(1)
            a.diffuse_step()
            b.step(1)
        alive = a.diffuse_count()[0]
        state = a.download(pressure=True)
        print("read-only: solver %d, %d diffuse particles, fluid finite %s" % (solver, alive, bool(np.isfinite(state[1]).all())))
        assert alive > 0 or not np.isfinite(state[1]).all(), solver  # (the diffuse steps did run on something)
        for x, y in zip(state, b.download(pressure=True)):
            assert x.tobytes() == y.tobytes(), solver
        a.close()
        b.close()


def test_sampler_results_and_build_count():
    s = dam_solver(False, capi.MULLER)
    fpos, _ = s.download()
    s.diffuse_configure(**dm.config(capacity=1 << 14, **SETTINGS))
    q = np.ones((50, 4), np.float32)
    q[:, :3] = np.random.default_rng(8).uniform(fpos[:, :3].min(0), fpos[:, :3].max(0), (50, 3))
    builds = s.sample_builds()
    s.sample_points(q, capi.FIELD_DENSITY | capi.FIELD_VELOCITY | capi.FIELD_GRADIENT)
    assert s.sample_builds() == builds + 1
    before = [s.sample_result(f) for f in (capi.FIELD_DENSITY, capi.FIELD_VELOCITY, capi.FIELD_GRADIENT)]
    s.diffuse_step()
    assert s.sample_builds() == builds + 1  # the same state: the sampler's grid serves
    after = [s.sample_result(f) for f in (capi.FIELD_DENSITY, capi.FIELD_VELOCITY, capi.FIELD_GRADIENT)]
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes() and x.any()
    refused(E_STATE, lambda: s.sample_result(capi.FIELD_COUNT))  # (still the result of the sample call, not of the diffuse step)
    s.step(1)
    s.diffuse_step()
    assert s.sample_builds() == builds + 2
    s.diffuse_step()
    assert s.sample_builds() == builds + 2
    s.close()


# ---- 6. reproducibility ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_same_seed_same_bytes(double, ks):
    out = []
    for seed in (5, 5, 6):
        s = dam_solver(double, ks)
        c = dict(SETTINGS, seed=seed)
        s.diffuse_configure(**dm.config(capacity=1 << 14, **c))
        for k in range(3):
            s.diffuse_step()
        out.append([s.diffuse_result(w) for w in (POS, VEL, KIND, POT, NORMALS, BIRTHS)] + [s.diffuse_count()])
        s.close()
    a, b, c = out
    assert len(a[0]) > 100
    for x, y in zip(a[:6], b[:6]):
        assert x.tobytes() == y.tobytes()
    assert a[6] == b[6]
    assert a[3].tobytes() == c[3].tobytes() and a[4].tobytes() == c[4].tobytes()  # potentials and normals do not depend on the seed
    assert a[0].shape != c[0].shape or a[0].tobytes() != c[0].tobytes()


# ---- 7. empty cases and refusals ------------------------------------------------------------------------------------------------------------------------
def test_empty_cases():
    s = dam_solver(False, capi.MULLER)
    p, real = s.params, s.real
    fpos, fvel = s.download()
    # all clamp ranges above every potential: nothing is born
    s.diffuse_configure(**dm.config(capacity=64, **dict(SETTINGS, tau_ta=(1e3, 2e3), tau_wc=(1e3, 2e3), tau_k=(1e3, 2e3))))
    s.diffuse_step()
    assert not s.diffuse_result(BIRTHS).any() and len(s.diffuse_result(BIRTHS)) == len(fpos) and s.diffuse_count() == (0, [0, 0, 0], 0)
    assert not s.diffuse_result(POT)[:, :3].any() and s.diffuse_result(NORMALS).any()
    assert s.diffuse_result(POS).shape == (0, 4) and s.diffuse_device_ptr(POS) == (None, 0)
    # release, then a step works again from an empty set
    s.diffuse_configure(**dm.config(capacity=1 << 14, **SETTINGS))
    s.diffuse_step()
    n1 = s.diffuse_count()[0]
    assert n1 > 0
    s.diffuse_release()
    assert s.diffuse_count() == (0, [0, 0, 0], 0)
    refused(E_STATE, lambda: s.diffuse_result(POT))
    s.diffuse_step()
    r = dm.step(p, dm.config(capacity=1 << 14, **SETTINGS), fpos, fvel, np.zeros((0, 4), real), np.zeros((0, 4), real), 1, 0.0)
    check_step(s, r, "after release")
    s.close()
    # no fluid: nothing is born and the survivors fly as spray
    p0, sc = small_dam_break((12, 10, 9))
    t = capi.Solver(p0, 16, solver=capi.SESPH)
    cfg = dm.config(capacity=8, **SETTINGS)
    t.diffuse_configure(**cfg)
    up = np.array([[0.1, 0.2, 0.3, 1.0], [0.5, 0.5, 0.5, 2.0]], np.float32)
    uv = np.array([[0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]], np.float32)
    t.diffuse_upload(up, uv)
    t.diffuse_step()
    r = dm.step(t.params, cfg, np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), up, uv, 0, 0.0)
    assert r["alive"] == 2 and list(r["kind"]) == [0, 0]
    pos, vel, kind = device_set(t)
    same(pos, r["pos"], "no fluid positions")
    same(vel, r["vel"], "no fluid velocities")
    assert t.diffuse_count() == (2, [2, 0, 0], 0) and t.diffuse_result(BIRTHS).shape == (0,)
    t.close()


def test_refusals():
    p, sc = small_dam_break((12, 10, 9))
    s = capi.Solver(p, len(sc["pos"]), solver=capi.SESPH)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    good = dm.config(capacity=256, **SETTINGS)
    # before configure; the argument's fault is named before the state's
    refused(E_STATE, lambda: s.diffuse_step())
    refused(E_INVALID, lambda: s.diffuse_step(-1.0))
    refused(E_INVALID, lambda: s.diffuse_step(float("nan")))
    refused(E_STATE, lambda: s.diffuse_count())
    refused(E_STATE, lambda: s.diffuse_result(POS))
    refused(E_INVALID, lambda: s.diffuse_result(6))
    refused(E_STATE, lambda: s.diffuse_upload(np.zeros((1, 4)), np.zeros((1, 4))))
    for bad in (dict(capacity=0), dict(tau_ta=(1.0, 1.0)), dict(k_drag=1.5), dict(max_per_particle=0), dict(struct_size=64), dict(reserved=1),
                dict(lifetime=(2.0, 1.0))):
        refused(E_INVALID, lambda: s.diffuse_configure(**dict(good, **bad)))
    refused(E_STATE, lambda: s.diffuse_step())  # (a refused configure configures nothing)
    s.diffuse_configure(**good)
    assert s.diffuse_count() == (0, [0, 0, 0], 0)
    refused(E_STATE, lambda: s.diffuse_result(POT))
    refused(E_INVALID, lambda: s.diffuse_upload(np.zeros((257, 4)), np.zeros((257, 4))))
    refused(E_INVALID, lambda: s.diffuse_step(-1e-3))
    s.diffuse_step(5e-4)
    assert s.diffuse_count() == (0, [0, 0, 0], 0) and len(s.diffuse_result(BIRTHS)) == len(sc["pos"])  # (the fluid rests: nothing is born)
    # mid-update after a partial step
    s.step_partial(capi.STAGE_DENSITY)
    refused(E_STATE, lambda: s.diffuse_step())
    refused(E_INVALID, lambda: s.diffuse_step(float("inf")))
    s.set_particles(sc["pos"], sc["vel"])
    s.diffuse_step()
    # a grid the walk cannot serve
    base = s.params.copy()
    q = base.copy()
    q["cellSize"][0] = (0.9 * float(p["interactionRadius"][0]),) * 3
    s.set_params(q)
    refused(E_INVALID, lambda: s.diffuse_step())
    s.set_params(base)
    s.diffuse_step()
    # a slab context
    s.slab_configure(0, 64, 8)
    refused(E_INVALID, lambda: s.diffuse_step())
    refused(E_INVALID, lambda: s.diffuse_configure(**good))
    s.close()
    # a host-driven IISPH step in progress
    p2, sc2 = small_dam_break((12, 10, 9), solver=capi.IISPH)
    t = capi.Solver(p2, len(sc2["pos"]), solver=capi.IISPH)
    t.set_particles(sc2["pos"], sc2["vel"])
    t.set_boundaries(sc2["bi"], sc2["vbi"], update_grid=True)
    t.diffuse_configure(**good)
    t.iisph_predict()
    refused(E_STATE, lambda: t.diffuse_step())
    t.iisph_iterate()
    t.iisph_finish()
    t.diffuse_step()
    t.close()
