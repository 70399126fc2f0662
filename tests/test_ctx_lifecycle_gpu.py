"""A context's whole life, repeated in one process: every buffer, pinned landing and event of the context frees itself (DevBuf,
PinnedBuf, Event in nereus_amd/csrc/nrs_ctx_base.h), so creating, using and destroying contexts over and over must neither disturb
one another nor change a result.  Every call here is a valid call.

Scenes: the plate scene of tests/test_bodies_gpu.py (tests/common.plate_scene: small_dam_break in its boundary box plus three kinematic bodies) for the five
solvers with every optional part switched on; tests/common.small_dam_break itself for the histogram and the pending snapshot."""
import ctypes as C

import numpy as np
import pytest

from nereus_amd import capi
from tests.common import SOLVER_NAMES, SOLVERS, plate_scene, plate_solver, small_dam_break

pytestmark = pytest.mark.gpu
REPEATS, STEPS = 5, 3


def destroy(s):
    """nrs_destroy with its return value (Solver.close drops it)"""
    rc = s.lib.nrs_destroy(s.h)
    s.h = None
    return rc


def one_life(solver):
    s = plate_solver(plate_scene(), solver)  # bodies assigned, the plate, the dot and the bar moving
    if solver in (capi.PCISPH, capi.PBF, capi.DFSPH):
        s.surface_akinci(1.0, 1.0)
    if solver == capi.PBF:
        s.pbf_set_tensile(1e-3, 0.3)
        s.pbf_set_vorticity(0.5)
    s.set_profiling(True)
    s.step(STEPS)
    s.snapshot_begin(with_vel=True)
    spos, svel, sstep = s.snapshot_wait()
    spos, svel = spos.copy(), svel.copy()  # (views of the context's pinned memory)
    ms, cnt = C.c_float(0), C.c_uint32(0)
    s._chk(s.lib.nrs_stage_ms(s.h, capi.STAGE_REORDER, C.byref(ms), C.byref(cnt)))
    pos, vel = s.download()
    assert destroy(s) == 0
    assert sstep == STEPS and cnt.value == STEPS and ms.value > 0.0
    np.testing.assert_array_equal(spos, pos)
    np.testing.assert_array_equal(svel, vel)
    return pos, vel


@pytest.mark.parametrize("solver", SOLVERS, ids=[SOLVER_NAMES[k] for k in SOLVERS])
def test_repeated_lives_are_bitwise_equal(hip_lib, solver):
    first = one_life(solver)
    assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all()
    for rep in range(1, REPEATS):
        pos, vel = one_life(solver)
        np.testing.assert_array_equal(pos, first[0], err_msg="positions, repetition %d" % (rep + 1))
        np.testing.assert_array_equal(vel, first[1], err_msg="velocities, repetition %d" % (rep + 1))


def plain_context():
    p, sc = small_dam_break()
    s = capi.Solver(p, len(sc["pos"]), solver=capi.SESPH)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    return s


def test_histogram_on_a_context_without_slabs(hip_lib):
    s = plain_context()
    s.step(1)
    columns = int(s.params["gridSize"][0][0])
    for _ in range(3):
        counts = s.slab_histogram(0, columns)
        assert counts.shape == (columns,) and int(counts.sum()) == s.n
    assert destroy(s) == 0


def test_destroy_with_a_snapshot_in_flight(hip_lib):
    s = plain_context()
    s.step(1)
    s.snapshot_begin(with_vel=True)  # (no wait: the destroy finds it pending)
    assert destroy(s) == 0
    t = plain_context()
    t.step(2)
    pos, vel = t.download()
    assert np.isfinite(pos).all() and np.isfinite(vel).all()
    assert destroy(t) == 0
