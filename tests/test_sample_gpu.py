"""The field sampler on the device (include/nereus_hip.h "field sampling"; DESIGN.md "Field sampling") against the brute-force model of
tests/sample_model.py, whose docstring derives the tolerance: counts and cut-off decisions exact, every sum within k * eps * sum|term|.

Measured max(error / bound) over all cases of this file in the four builds (MI355X): density 0.33, gradient 0.33, velocity 0.33
(DESIGN.md "Field sampling").
"""
import ctypes as C

import numpy as np
import pytest

from nereus_amd import capi
from nereus_amd.params import default_params
from tests import sample_model as sm
from tests.common import plate_scene, plate_solver, small_dam_break

pytestmark = pytest.mark.gpu

BUILDS = [(False, capi.MULLER), (False, capi.MONAGHAN), (True, capi.MULLER), (True, capi.MONAGHAN)]
BUILD_IDS = ["f32-muller", "f32-monaghan", "f64-muller", "f64-monaghan"]
OUT = [capi.FIELD_DENSITY, capi.FIELD_GRADIENT, capi.FIELD_VELOCITY, capi.FIELD_COUNT]
ALL = sum(OUT)
E_INVALID, E_STATE = -1, -4


def results(s, fields=ALL):
    return {f: s.sample_result(f) for f in OUT if fields & f}


def same_bytes(a, b, what=""):
    assert a.keys() == b.keys()
    for f in a:
        assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape, (what, f)
        assert a[f].tobytes() == b[f].tobytes(), (what, "field %d differs between the two entry points" % f)


def refused(s, code, call):
    with pytest.raises(capi.NereusError) as e:
        call()
    assert ("error %d:" % code) in str(e.value), str(e.value)
    assert len(str(e.value).split(":", 1)[1].strip()) > 0  # (a text for nrs_last_error)


# ---- the shared state: the small dam break after three steps, one per build -----------------------------------------------------------
_states = {}


def dam_state(double, ks):
    """(solver, params, h, downloaded pos, vel, sorted boundary array) of small_dam_break((12, 10, 9)) after nrs_step(ctx, 3)"""
    key = (double, ks)
    if key not in _states:
        p, sc = small_dam_break((12, 10, 9), double=double, kernel_set=ks)
        rng = np.random.default_rng(11)
        vel = sc["vel"].copy()
        vel[:, :3] = rng.uniform(-0.3, 0.3, (len(vel), 3))
        s = capi.Solver(p, len(sc["pos"]), solver=capi.SESPH, double=double, kernel_set=ks)
        s.set_particles(sc["pos"], vel)
        s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
        s.step(3)
        pos, v = s.download()
        assert len(pos) == 1080 and np.abs(v[:, :3]).min() > 0
        _states[key] = (s, s.params, float(p["interactionRadius"][0]), pos, v, s.get("bSorted"))
    return _states[key]


def box_points(rng, pos, h, n, real):
    lo, hi = pos[:, :3].astype(np.float64).min(0) - 2 * h, pos[:, :3].astype(np.float64).max(0) + 2 * h
    q = np.ones((n, 4), real)
    q[:, :3] = rng.uniform(lo, hi, (n, 3)).astype(real)
    return q


# ---- 1. points against the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_points_match_model(double, ks):
    s, p, h, pos, vel, bs = dam_state(double, ks)
    real = s.real
    q = box_points(np.random.default_rng(5), pos, h, 777, real)
    q[0] = pos[417]                                                   # a particle's position, bit for bit
    q[1, :3] = (float(p["worldOrigin"][0][0]) - 0.3 * h, float(pos[:, 1].mean()), float(pos[:, 2].mean()))  # its cells wrap in x
    q[2, 1] = np.nan
    q[3, 0] = np.inf
    assert len(q) % 64 != 0 and len(q) % 256 != 0
    for walls in (0, capi.FIELD_WALLS):
        s.sample_points(q, ALL | walls)
        got = results(s)
        want = sm.sample(p, pos, vel, q, ks, bs if walls else None)
        assert want["count"][0] >= 1 and (want["count"] == 0).sum() > 4 and want["count"].max() > 5
        sm.compare(got, want, "points %s walls=%d" % (BUILD_IDS[BUILDS.index((double, ks))], walls))
        for f in OUT:   # the non-finite queries: zeros, count 0
            assert not got[f][2:4].any()
        if walls:
            assert (want["k"] > want["count"]).any()  # (some queries do see the wall)


# ---- 2. lattice == points, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_lattice_equals_points(double, ks):
    s, p, h, pos, vel, bs = dam_state(double, ks)
    lo = pos[:, :3].astype(np.float64).min(0)
    origin = (float(p["worldOrigin"][0][0]) - 0.25 * h, lo[1] - h, lo[2] - h)  # starts below the grid's low corner in x, outside the fluid
    dims = (13, 7, 5)
    nodes = sm.lattice_points(origin, h / 2, dims, s.real)
    for walls in (0, capi.FIELD_WALLS):
        s.sample_lattice(origin, h / 2, dims, ALL | walls)
        a = results(s)
        s.sample_points(nodes, ALL | walls)
        b = results(s)
        same_bytes(a, b, "lattice vs points")
        want = sm.sample(p, pos, vel, nodes, ks, bs if walls else None)
        assert want["count"].max() > 4
        sm.compare(a, want, "lattice walls=%d" % walls)


# ---- 3. the smallest grid: 4 x 4 x 4 cells of size h ----------------------------------------------------------------------------------------
def tiny_grid_solver(double, ks, cells, pos):
    p = default_params(0, double)
    h = float(p["interactionRadius"][0])
    p["gridSize"][0] = (cells,) * 3
    p["numCells"][0] = cells ** 3
    p["worldOrigin"][0] = (0.0, 0.0, 0.0)
    p["cellSize"][0] = (p["interactionRadius"][0],) * 3
    s = capi.Solver(p, len(pos), solver=capi.SESPH, double=double, kernel_set=ks)
    s.set_particles(pos, np.zeros_like(pos))
    return s, s.params, h


@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_smallest_grid(double, ks):
    real = np.float64 if double else np.float32
    h = float(default_params(0, double)["interactionRadius"][0])
    rng = np.random.default_rng(3)
    pos = np.ones((300, 4), real)
    pos[:, :3] = rng.uniform(0.02 * h, 3.98 * h, (300, 3)).astype(real)
    s, p, h = tiny_grid_solver(double, ks, 4, pos)
    vel = np.zeros_like(pos)
    origin, dims = (-h, -h, -h), (13, 13, 13)  # the box and one cell beyond on every side, at h / 2
    s.sample_lattice(origin, h / 2, dims, ALL)
    a = results(s)
    nodes = sm.lattice_points(origin, h / 2, dims, real)
    s.sample_points(nodes, ALL)
    same_bytes(a, results(s), "smallest grid")
    want = sm.sample(p, pos, vel, nodes, ks)
    sm.compare(a, want, "smallest grid")  # (counts equal the model's: nothing is counted twice through the wrap)


# ---- 4. a dense cell: a run longer than one 64-candidate load -----------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
def test_dense_cell(double):
    real = np.float64 if double else np.float32
    h = float(default_params(0, double)["interactionRadius"][0])
    rng = np.random.default_rng(8)
    dense = rng.uniform(3.02 * h, 3.98 * h, (200, 3))
    sparse = rng.uniform(2.0 * h, 5.0 * h, (150, 3))
    pos = np.ones((350, 4), real)
    pos[:, :3] = np.concatenate([dense, sparse]).astype(real)
    assert len(np.unique(pos[:, :3], axis=0)) == 350
    s, p, h = tiny_grid_solver(double, capi.MULLER, 8, pos)
    vel = np.zeros_like(pos)
    vel[:, :3] = rng.uniform(-1, 1, (350, 3)).astype(real)
    s.set_particles(pos, vel)
    origin, dims = (1.5 * h,) * 3, (9, 9, 9)
    s.sample_lattice(origin, h / 2, dims, ALL)
    a = results(s)
    nodes = sm.lattice_points(origin, h / 2, dims, real)
    s.sample_points(nodes, ALL)
    same_bytes(a, results(s), "dense cell")
    want = sm.sample(p, pos, vel, nodes, capi.MULLER)
    assert want["count"].max() > 128
    sm.compare(a, want, "dense cell")


# ---- 5. a mostly empty lattice ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_mostly_empty_lattice(double, ks):
    s, p, h, pos, vel, bs = dam_state(double, ks)
    origin = tuple(pos[:, :3].astype(np.float64).min(0) - 1.5 * h)
    dims = (40, 40, 40)
    s.sample_lattice(origin, h, dims, ALL)
    got = results(s)
    want = sm.sample(p, pos, vel, sm.lattice_points(origin, h, dims, s.real), ks)
    empty = want["count"] == 0
    assert empty.mean() > 0.8 and (~empty).sum() > 500
    assert not got[capi.FIELD_DENSITY][empty].any() and not got[capi.FIELD_GRADIENT][empty].any() and not got[capi.FIELD_VELOCITY][empty].any()
    assert np.all(got[capi.FIELD_DENSITY][~empty] > 0)
    sm.compare(got, want, "mostly empty lattice")


# ---- 6. read-only: a context that samples steps bit-identically to one that never did ------------------------------------------------------------
@pytest.mark.parametrize("solver,lattice", [(capi.SESPH, (33, 32, 32)), (capi.SESPH, (12, 10, 9)), (capi.DFSPH, (12, 10, 9)), (capi.DFSPH, (13, 9, 8))],
                         ids=["sesph-resort", "sesph-small", "dfsph", "dfsph-odd"])
def test_sampling_changes_no_step(solver, lattice):
    p, sc = small_dam_break(lattice)
    h = float(p["interactionRadius"][0])
    assert solver != capi.SESPH or lattice != (33, 32, 32) or len(sc["pos"]) >= 32768  # RESORT_MIN_PARTICLES: the coherent re-sort is live
    pair = []
    for k in range(2):
        s = capi.Solver(p, len(sc["pos"]), solver=solver)  # the production flags
        s.set_particles(sc["pos"], sc["vel"])
        s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
        pair.append(s)
    a, b = pair
    a.step(3)
    q = box_points(np.random.default_rng(1), sc["pos"], h, 500, np.float32)
    a.sample_points(q, ALL | capi.FIELD_WALLS)
    a.sample_lattice(tuple(sc["pos"][:, :3].min(0) - h), h / 2, (17, 9, 6), ALL)
    assert a.sample_result(capi.FIELD_COUNT).max() > 0
    a.step(2)
    b.step(5)
    if solver == capi.SESPH and len(sc["pos"]) >= 32768:
        assert a.resort_stats() == b.resort_stats() and a.resort_stats()[0] > 0
    for x, y in zip(a.download(pressure=True), b.download(pressure=True)):
        assert x.tobytes() == y.tobytes()
    a.close()
    b.close()


# ---- 7. a moving wall: the wall term follows the pose ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_wall_term_follows_the_pose(double, ks):
    sc = plate_scene(double, ks)
    s = plate_solver(sc, capi.SESPH, double=double, kernel_set=ks)
    s.step(2)
    pos, vel = s.download()
    bs, body = s.get("bSorted"), s.get("b_body")
    h = float(sc[0]["interactionRadius"][0])
    plate = bs[body == 1]
    assert len(plate) == 165
    rest_x = float(sc[6][1][0, 0])
    assert abs(float(plate[0, 0]) - (rest_x + 2 * 9.0 * 1e-3)) < 1e-5  # the plate has moved two steps of 9 m/s
    rng = np.random.default_rng(2)
    q = np.ones((333, 4), s.real)
    q[:, :3] = (plate[rng.integers(0, len(plate), 333), :3].astype(np.float64) + rng.uniform(-0.6 * h, 0.6 * h, (333, 3))).astype(s.real)
    fields = capi.FIELD_DENSITY | capi.FIELD_COUNT | capi.FIELD_WALLS
    s.sample_points(q, fields)
    want = sm.sample(s.params, pos, vel, q, ks, bs)
    assert (want["k"] > want["count"]).mean() > 0.9
    sm.compare(results(s, fields), want, "moving wall")
    s.close()


# ---- 8. cache and lifetime ------------------------------------------------------------------------------------------------------------------------------
def test_cache_and_lifetime():
    p, sc = small_dam_break((12, 10, 9))
    h = float(p["interactionRadius"][0])
    s = capi.Solver(p, len(sc["pos"]), solver=capi.PCISPH)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    assert s.sample_builds() == 0
    refused(s, E_STATE, lambda: s.sample_result(capi.FIELD_DENSITY))  # before any call
    q = box_points(np.random.default_rng(4), sc["pos"], h, 300, np.float32)
    s.sample_points(q, ALL)
    first = results(s)
    s.sample_lattice((0.0, 0.0, 0.0), h / 2, (9, 9, 9), capi.FIELD_DENSITY)
    assert s.sample_builds() == 1
    refused(s, E_STATE, lambda: s.sample_result(capi.FIELD_COUNT))    # the last call did not compute it
    ptr, nbytes = s.sample_device_ptr(capi.FIELD_DENSITY)
    assert ptr and nbytes == 4 * 729
    s.sample_points(q, ALL)
    same_bytes(first, results(s), "two runs of one call")
    assert s.sample_builds() == 1
    s.step(1)
    s.sample_points(q, ALL)
    assert s.sample_builds() == 2
    after = results(s)
    assert after[capi.FIELD_VELOCITY].tobytes() != first[capi.FIELD_VELOCITY].tobytes()
    s.sample_release()
    refused(s, E_STATE, lambda: s.sample_result(capi.FIELD_DENSITY))
    refused(s, E_STATE, lambda: s.sample_device_ptr(capi.FIELD_DENSITY))
    s.sample_points(q, ALL)
    same_bytes(after, results(s), "after release")
    assert s.sample_builds() == 3
    s.set_particles(sc["pos"], sc["vel"])                              # an upload: the grid is built again, on the first state
    s.sample_points(q, ALL)
    same_bytes(first, results(s), "after an upload")
    assert s.sample_builds() == 4
    s.sample_points(np.zeros((0, 4), np.float32), ALL)                 # m == 0: a successful no-op with empty results
    assert all(len(v) == 0 for v in results(s).values())
    s.set_particles(np.zeros((0, 4), np.float32))                      # n == 0: zeros
    s.sample_points(q, ALL)
    assert not any(v.any() for v in results(s).values())
    s.close()


# ---- 9. refusals at the ABI, each leaving the context usable -------------------------------------------------------------------------------------------
def test_refusals():
    p, sc = small_dam_break((12, 10, 9))
    h = float(p["interactionRadius"][0])
    s = capi.Solver(p, len(sc["pos"]), solver=capi.SESPH)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    q = box_points(np.random.default_rng(6), sc["pos"], h, 100, np.float32)
    s.sample_points(q, ALL)
    good = results(s)

    def usable():
        s.sample_points(q, ALL)
        same_bytes(good, results(s), "after a refusal")

    for fields in (0, capi.FIELD_WALLS, 32, ALL | 64):
        refused(s, E_INVALID, lambda: s.sample_points(q, fields))
        refused(s, E_INVALID, lambda: s.sample_lattice((0, 0, 0), h, (2, 2, 2), fields))
    refused(s, E_INVALID, lambda: s._chk(s.lib.nrs_sample_points(s.h, None, 5, ALL)))
    refused(s, E_INVALID, lambda: s._chk(s.lib.nrs_sample_lattice(s.h, None, ALL)))
    for spacing in (0.0, -h, np.nan, np.inf, (h, h, 0.0)):
        refused(s, E_INVALID, lambda: s.sample_lattice((0, 0, 0), spacing, (2, 2, 2), ALL))
    for dims in ((0, 2, 2), (2, 2, 0), (2048, 2048, 513), (65536, 65536, 1), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)):
        refused(s, E_INVALID, lambda: s.sample_lattice((0, 0, 0), h, dims, ALL))
    refused(s, E_INVALID, lambda: s.sample_result(3))
    usable()
    # mid-update after a partial step
    s.step_partial(capi.STAGE_DENSITY)
    refused(s, E_STATE, lambda: s.sample_points(q, ALL))
    refused(s, E_STATE, lambda: s.sample_lattice((0, 0, 0), h, (2, 2, 2), ALL))
    s.set_particles(sc["pos"], sc["vel"])
    usable()
    # a grid the 27-cell walk does not cover, or whose rows alias
    base = s.params
    for name, val in (("cellSize", (0.9 * h, h, h)), ("gridSize", (2, 64, 64)), ("gridSize", (64, 48, 64))):
        bad = base.copy()
        bad[name][0] = val
        bad["numCells"][0] = int(np.prod(bad["gridSize"][0]))
        s.set_params(bad)
        refused(s, E_INVALID, lambda: s.sample_points(q, ALL))
        s.set_params(base)
        usable()
    # a slab context
    s.slab_configure(0, 64, 8)
    refused(s, E_INVALID, lambda: s.sample_points(q, ALL))
    assert len(s.download()[0]) == len(sc["pos"])
    s.close()
    # a host-driven IISPH step in progress
    p2, sc2 = small_dam_break((12, 10, 9), solver=capi.IISPH)
    t = capi.Solver(p2, len(sc2["pos"]), solver=capi.IISPH)
    t.set_particles(sc2["pos"], sc2["vel"])
    t.set_boundaries(sc2["bi"], sc2["vbi"], update_grid=True)
    t.iisph_predict()
    refused(t, E_STATE, lambda: t.sample_points(q, ALL))
    t.iisph_iterate()
    t.iisph_finish()
    t.sample_points(q, ALL)
    assert t.sample_result(capi.FIELD_COUNT).max() > 0
    t.close()


# ---- 10. queued steps: the sample call waits for the steps handed to the worker -----------------------------------------------------------------------
@pytest.mark.parametrize("double,ks", BUILDS, ids=BUILD_IDS)
def test_sample_behind_queued_steps(double, ks):
    p, sc = small_dam_break((12, 10, 9), double=double, kernel_set=ks)
    h = float(p["interactionRadius"][0])
    s = capi.Solver(p, len(sc["pos"]), solver=capi.SESPH, double=double, kernel_set=ks)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    origin, dims = tuple(sc["pos"][:, :3].astype(np.float64).min(0) - h), (11, 9, 7)
    s.step(4)
    s.sample_lattice(origin, h / 2, dims, ALL)
    got = results(s)
    pos, vel = s.download()
    want = sm.sample(s.params, pos, vel, sm.lattice_points(origin, h / 2, dims, s.real), ks)
    sm.compare(got, want, "behind queued steps")
    t = capi.Solver(p, len(sc["pos"]), solver=capi.SESPH, double=double, kernel_set=ks)
    t.set_particles(sc["pos"], sc["vel"])
    t.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    for _ in range(4):
        t.step(1)
    for x, y in zip(t.download(), (pos, vel)):
        assert x.tobytes() == y.tobytes()
    s.close()
    t.close()
