"""Kinematic boundary bodies on the device (nrs_set_boundary_bodies, DESIGN.md "Kinematic boundary bodies"): the transform against
the float64 model, bodies that do not move, equivalence with re-uploading the walls, list-driven against reference-order kernels
while a plate crosses cell faces, DFSPH's wall-velocity term against the model, queued steps, a piston, and the refusals.

Scene: tests/common.small_dam_break moved three cells away from the wall x = 0, inside its boundary box (body 0), plus body 1, a
plate of 15 x 11 boundary particles at fluid spacing between that wall and the fluid, body 2, a single particle, and body 3, a bar of
7 particles that rotates.  nb = 7987, no multiple of the workgroup size."""
import re

import numpy as np
import pytest

from nereus_amd import capi
from tests import bodies_model as bm
from tests import dfsph_model
from tests.common import BAR_W, DOT_V, PLATE_V, SOLVER_NAMES as NAMES, SOLVERS, check_cell_tables, rel_err, small_dam_break
from tests.common import plate_scene as scene, plate_solver as make

pytestmark = pytest.mark.gpu


def unsorted_walls(s):
    """the boundary particles of the last step in upload order, (nb, 4)"""
    bs, idx = s.get("bSorted"), s.get("bindex")
    out = np.empty_like(bs)
    out[idx] = bs
    return out


def state(s, tables=False):
    o = {"pos": s.get("pos"), "vel": s.get("vel")}
    if tables:
        for k in ("bhash", "bindex", "bSorted", "bCellStart", "bCellEnd"):
            o[k] = s.get(k)
    return o


def same(a, b, what):
    for k in a:
        if k in ("bCellStart", "bCellEnd"):
            continue
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s %s" % (what, k))
    if "bCellStart" in a:
        check_cell_tables(a["bCellStart"], a["bCellEnd"], b["bCellStart"], b["bCellEnd"])


# ---- 1. the transform against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [False, True])
def test_transform_matches_model(hip_lib, double):
    sc = scene(double)
    p, pos, vel, bi, vbi, body_of, parts = sc
    real = np.float64 if double else np.float32
    s = make(sc, capi.SESPH, double=double)
    vel_of = {1: ((1.5, 0.2, -0.1), (0.0, 0.0, 0.0)), 2: (DOT_V, (0.0, 0.0, 0.0)), 3: ((0.3, -0.2, 0.1), (4.0, -9.0, 30.0))}
    model = {}
    for k, (v, w) in vel_of.items():
        s.set_body_velocity(k, v, w)
        model[k] = bm.Body(parts[k], v, w)
    dt = float(p["timestep"][0])
    for step in range(20):
        if step == 11:   # the time step changes once mid-run
            q = s.params.copy()
            q["timestep"] = real(0.6 * dt)
            s.set_params(q)
            dt = float(q["timestep"][0])
        s.step(1)
        for b in model.values():
            b.step(dt)
    world = unsorted_walls(s)
    np.testing.assert_array_equal(s.get("b_body")[np.argsort(s.get("bindex"))], body_of)
    np.testing.assert_array_equal(world[body_of == 0], np.concatenate([parts[0][:, :3], vbi[body_of == 0, None]], axis=1))
    np.testing.assert_array_equal(world[:, 3], vbi)
    for k, b in model.items():
        x, q = s.body_pose(k)
        print("body %d pose error %.3g %.3g" % (k, np.abs(x - b.x).max(), np.abs(q - b.q).max()))
        assert np.abs(x - b.x).max() <= 1e-12 and np.abs(q - b.q).max() <= 1e-12
        want, bound = b.world(real)
        err = np.abs(world[body_of == k, :3].astype(np.float64) - want)
        print("body %d: max error / bound %.3g" % (k, (err / bound).max()))
        assert np.all(err <= bound), (k, (err / bound).max())
    assert np.abs(model[3].q - [1, 0, 0, 0]).max() > 0.1     # the bar really turned
    s.close()


# ---- 2. defined but not moving ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=[NAMES[k] for k in SOLVERS])
def test_bodies_at_rest_change_nothing(hip_lib, solver):
    sc = scene()
    got = []
    for bodies in (False, True):
        s = make(sc, solver, bodies=bodies, moving=False)
        s.step(5)
        got.append(state(s, tables=True))
        s.close()
    same(got[0], got[1], NAMES[solver])


# ---- 3. equivalence with re-uploading the walls ----------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,double,kernel_set", [(capi.SESPH, False, capi.MULLER), (capi.IISPH, False, capi.MULLER),
                                                      (capi.PCISPH, False, capi.MULLER), (capi.PBF, False, capi.MULLER),
                                                      (capi.PCISPH, True, capi.MONAGHAN)],
                         ids=["sesph", "iisph", "pcisph", "pbf", "pcisph-f64-monaghan"])
def test_device_motion_equals_reupload(hip_lib, solver, double, kernel_set):
    sc = scene(double, kernel_set)
    a = make(sc, solver, double=double, kernel_set=kernel_set)
    b = make(sc, solver, bodies=False, double=double, kernel_set=kernel_set)
    rest = a.get("bhash")
    for step in range(10):
        a.step(1)
        w = unsorted_walls(a)   # the pose of A's step, handed to B before its step
        b.set_boundaries(w, w[:, 3].copy(), update_grid=False)
        b.step(1)
        same(state(a, tables=True), state(b, tables=True), "step %d" % step)
    assert not np.array_equal(rest, a.get("bhash"))
    a.close()
    b.close()


# ---- 4. list-driven kernels against reference order while the plate crosses cell faces -----------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=[NAMES[k] for k in SOLVERS])
def test_list_kernels_equal_reference_order_with_moving_walls(hip_lib, solver):
    sc = scene()
    p = sc[0]
    steps = 12
    ref = make(sc, solver, reference_order=True)
    # (1,080 particles never re-sort coherently, so the FLAG_FULL_SORT run is the default run here: tests/test_resort_features_gpu.py has the tank-scale one)
    runs = [make(sc, solver), make(sc, solver, flags=capi.FLAG_NO_WALL_WORKGROUPS), make(sc, solver, flags=capi.FLAG_FULL_SORT)]
    if solver == capi.SESPH:   # the LDS-staged density launch while the plate crosses cell faces and the boundary tables are rebuilt
        runs.append(make(sc, solver, flags=capi.FLAG_STAGED_SCAN))
    h, ox = float(p["interactionRadius"][0]), float(ref.params["worldOrigin"][0][0])
    cells, reach = set(), 0
    for step in range(steps):
        ref.step(1)
        want = state(ref, tables=True)
        px = ref.body_pose(1)[0][0]
        cells.add(int(np.floor((px - ox) / h)))
        reach += bool(px > float(want["pos"][:, 0].min()) - h)
        for k, s in enumerate(runs):
            s.step(1)
            same(state(s, tables=True), want, "%s run %d step %d" % (NAMES[solver], k, step))
    assert len(cells) >= 3, cells     # the plate crossed two cell faces
    assert reach >= 2, reach          # ... into reach of fluid particles, for at least two of the steps
    for s in runs + [ref]:
        s.close()


# ---- 5. DFSPH: the wall velocity in launch A -----------------------------------------------------------------------------------------
def _dfsph_stages(sc, double, kernel_set, reference_order, plate_v):
    cfg = (0.0, 3, 0.0, 3, 1)
    o = {}

    def ctx():
        p, pos, vel, bi, vbi, body_of, _ = sc
        k = np.arange(len(vel))
        v = vel.copy()
        v[:, 0] = 0.3 * np.sin(k)
        v[:, 1] = 0.3 * np.cos(0.7 * k)
        s = capi.Solver(p, len(pos), solver=capi.DFSPH, double=double, kernel_set=kernel_set, reference_order=reference_order)
        s.set_particles(pos, v)
        s.set_boundaries(bi, vbi, update_grid=True)
        s.dfsph_configure(*cfg)
        s.set_boundary_bodies(body_of, 4)
        s.set_body_velocity(1, plate_v)
        s.set_body_velocity(3, (0, 0, 0), BAR_W)
        return s

    s = ctx()
    s.step_partial(capi.STAGE_DENSITY)
    for k, nm in (("x", "sortedPos"), ("v0", "sortedVel"), ("rho", "dens"), ("alpha", "dfsphAlpha"), ("Kv_prev", "dfsphKappaV"),
                  ("K_prev", "pres"), ("bs", "bSorted"), ("body", "b_body")):
        o[k] = s.get(nm)
    o["pose"] = {k: s.body_pose(k) for k in (1, 2, 3)}
    s.close()
    s = ctx()
    s.step_partial(capi.STAGE_P_ADVECT)
    for k, nm in (("v_df", "sortedVel"), ("Kv", "dfsphKappaV"), ("velAdv0", "velAdv")):
        o[k] = s.get(nm)
    s.close()
    s = ctx()
    s.step_partial(capi.STAGE_P_SOLVE)
    for k, nm in (("vstar", "velAdv"), ("K", "pres"), ("kappa", "P_l"), ("rho_adv", "densCorr")):
        o[k] = s.get(nm)
    s.close()
    return o


@pytest.mark.parametrize("double,kernel_set,reference_order", [(False, capi.MULLER, False), (False, capi.MULLER, True),
                                                               (False, capi.MONAGHAN, False), (True, capi.MULLER, False),
                                                               (True, capi.MONAGHAN, False)],
                         ids=["f32-muller", "f32-muller-ref", "f32-monaghan", "f64-muller", "f64-monaghan"])
def test_dfsph_wall_velocity_term_matches_model(hip_lib, double, kernel_set, reference_order):
    tol = 1e-10 if double else 1e-4      # the bars of tests/test_dfsph_gpu.py, device against model
    h = 0.0457
    # (the Monaghan kernel, cut off at h, gives lower densities: a tighter column and a faster plate, so that the density solve has
    # particles above rest density next to the plate in both kernel sets)
    muller = kernel_set == capi.MULLER
    sc = scene(double, kernel_set, plate_gap=h - 0.005, squeeze=0.87 if muller else 0.75)
    p = sc[0]
    plate_v = (2.4, 0.0, 0.0) if muller else PLATE_V
    o = _dfsph_stages(sc, double, kernel_set, reference_order, plate_v)
    vel_of = {1: (plate_v, (0, 0, 0)), 2: ((0, 0, 0), (0, 0, 0)), 3: ((0, 0, 0), BAR_W)}
    bs = o["bs"].astype(np.float64)
    ub = np.zeros((len(bs), 3))
    for k, (v, w) in vel_of.items():
        m = o["body"] == k
        ub[m] = bm.wall_velocity(bs[m, :3], o["pose"][k][0], v, w)
    pairs = dfsph_model.Pairs(p, o["x"], o["bs"][:, :3], o["bs"][:, 3], kernel_set)
    assert (o["body"][pairs.bj] == 1).sum() > 50       # fluid particles have the plate among their neighbours
    alpha, _ = dfsph_model.factor(p, pairs, kernel_set)
    assert rel_err(o["alpha"], alpha) <= tol

    def run(moving):
        f = (lambda *a, **kw: bm.solve_moving(p, pairs, ub, *a, **kw)) if moving else (lambda *a, **kw: dfsph_model.solve(p, pairs, *a, **kw))
        div = f(alpha, o["v0"], o["Kv_prev"], min_iters=3, eta=0.0, warm=True)
        den = f(alpha, o["velAdv0"], o["K_prev"], rho=o["rho"], min_iters=3, eta=0.0, warm=True)
        return div, den

    div, den = run(True)
    assert (den["K"] > 0).any() and (div["K"] > 0).any()     # both solves have work to do
    errs = {"v_df": rel_err(o["v_df"][:, :3], div["u"]), "Kv": rel_err(o["Kv"], div["K"]), "vstar": rel_err(o["vstar"][:, :3], den["u"]),
            "K": rel_err(o["K"], den["K"]), "kappa": rel_err(o["kappa"], den["kappa"]), "rho_adv": rel_err(o["rho_adv"], den["rho_adv"])}
    print("with the term:", errs)
    div0, den0 = run(False)
    errs0 = {"v_df": rel_err(o["v_df"][:, :3], div0["u"]), "vstar": rel_err(o["vstar"][:, :3], den0["u"])}
    print("without it:", errs0)
    for k, e in errs.items():
        assert e <= tol, (k, e)
    for k, e in errs0.items():   # a kernel that ignored u_b could not pass the comparison above
        assert e > 100 * tol, (k, e)


# ---- 6. queued steps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [capi.SESPH, capi.DFSPH], ids=["sesph", "dfsph"])
def test_queued_steps_equal_single_steps(hip_lib, solver):
    sc = scene()
    a, b = make(sc, solver), make(sc, solver)
    a.step(6)
    for _ in range(6):
        b.step(1)
    a.synchronize()
    same(state(a, tables=True), state(b, tables=True), "queued")
    for k in (1, 2, 3):
        for u, v in zip(a.body_pose(k), b.body_pose(k)):
            np.testing.assert_array_equal(u, v)
    assert a.body_pose(1)[0][0] > scene()[6][1][0, 0] + 5.9 * PLATE_V[0] * 1e-3
    a.close()
    b.close()


# ---- 7. piston ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [capi.PBF, capi.DFSPH], ids=["pbf", "dfsph"])
def test_piston_pushes_the_fluid(hip_lib, solver):
    h = 0.0457
    sc = scene(plate_gap=h - 0.005)
    x0 = float(sc[1][:, 0].astype(np.float64).mean())
    com = []
    for v in ((2.4, 0.0, 0.0), None):     # two cell faces in 40 steps of 1 ms
        s = make(sc, solver, moving=False)
        if v:
            s.set_body_velocity(1, v)
        s.step(40)
        pos, vel = s.download()
        assert np.isfinite(pos).all() and np.isfinite(vel).all()
        com.append(float(pos[:, 0].astype(np.float64).mean()))
        s.close()
    print("centre of mass x: start %.6f, piston %.6f, plate at rest %.6f" % (x0, com[0], com[1]))
    assert com[0] > x0 and com[0] > com[1]


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def _code(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except capi.NereusError as e:
        return int(re.search(r"error (-?\d+)", str(e)).group(1))
    return 0


def test_refusals(hip_lib):
    E_INVALID, E_STATE = -1, -4
    sc = scene()
    p, pos, vel, bi, vbi, body_of, _ = sc
    s = capi.Solver(p, len(pos), solver=capi.SESPH)
    s.set_particles(pos, vel)
    assert _code(s.set_boundary_bodies, body_of, 4) == E_STATE          # before any nrs_set_boundaries
    s.set_boundaries(bi, vbi, update_grid=True)
    assert _code(s.get, "b_body") == E_STATE                            # no assignment yet
    assert _code(s.set_body_velocity, 1, (1, 0, 0)) == E_INVALID        # ... so no body is known
    assert _code(s.set_boundary_bodies, body_of[:-1], 4) == E_INVALID   # nb differs
    assert _code(s.set_boundary_bodies, body_of, 3) == E_INVALID        # an id >= nbodies
    assert _code(s.set_boundary_bodies, body_of, capi.MAX_BODIES + 1) == E_INVALID
    assert _code(s.set_boundary_bodies, body_of, 4) == 0
    assert _code(s.set_boundary_bodies, body_of, capi.MAX_BODIES) == 0  # (bodies without particles are allowed)
    assert _code(s.set_boundary_bodies, body_of, 4) == 0
    inf, nan = float("inf"), float("nan")
    assert _code(s.set_body_velocity, 0, (1, 0, 0)) == E_INVALID
    assert _code(s.set_body_velocity, 4, (1, 0, 0)) == E_INVALID
    assert _code(s.set_body_velocity, 1, (nan, 0, 0)) == E_INVALID
    assert _code(s.set_body_velocity, 1, (0, 0, 0), (0, inf, 0)) == E_INVALID
    assert _code(s.set_body_pose, 1, (0, 0, 0), (0, 0, 0, 0)) == E_INVALID
    assert _code(s.set_body_pose, 0, (0, 0, 0)) == E_INVALID
    assert _code(s.set_body_pose, 1, (nan, 0, 0)) == E_INVALID
    assert _code(s.body_pose, 0) == E_INVALID and _code(s.body_pose, 4) == E_INVALID
    assert _code(s.slab_configure, 0, 32, 2) == E_INVALID               # a context with bodies has no slabs
    # the quaternion is normalised; a teleport shows in the tables of the next step
    s.set_body_pose(2, (0.5, 0.3, 0.2), (2.0, 0.0, 0.0, 0.0))
    np.testing.assert_array_equal(s.body_pose(2)[1], [1.0, 0.0, 0.0, 0.0])
    s.step(1)
    np.testing.assert_array_equal(unsorted_walls(s)[body_of == 2, :3], np.array([[0.5, 0.3, 0.2]], np.float32))
    assert s.get("b_body").shape == body_of.shape
    # clearing puts the walls back where they were uploaded
    s.set_boundary_bodies(None, 0)
    assert _code(s.get, "b_body") == E_STATE
    np.testing.assert_array_equal(unsorted_walls(s)[:, :3], bi[:, :3])
    # a later nrs_set_boundaries clears the assignment
    s.set_boundary_bodies(body_of, 4)
    s.set_boundaries(bi, vbi, update_grid=False)
    assert _code(s.get, "b_body") == E_STATE
    assert _code(s.slab_configure, 0, 32, 2) == 0
    assert _code(s.set_boundary_bodies, body_of, 4) == E_INVALID        # a slab context
    s.close()
    # mid-IISPH-step
    s = capi.Solver(p, len(pos), solver=capi.IISPH)
    s.set_particles(pos, vel)
    s.set_boundaries(bi, vbi, update_grid=True)
    s.iisph_predict()
    assert _code(s.set_boundary_bodies, body_of, 4) == E_STATE
    s.iisph_iterate()
    s.iisph_iterate()
    s.iisph_finish()
    assert _code(s.set_boundary_bodies, body_of, 4) == 0
    s.close()
