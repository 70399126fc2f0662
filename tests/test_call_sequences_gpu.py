"""Call sequences that change the state of the particle arrays between steps (nrs_host_state.h: ArrayTracker, choose_sort_prefix,
choose_sort), on a scene large enough for the coherent re-sort: small_dam_break((34, 32, 32)) with its walls, fp32 Muller, 34,816
particles (RESORT_MIN_PARTICLES is 32,768), so a split of the next step's keys IS queued behind every full step.

Each test drives a default context and an NRS_FLAG_FULL_SORT context (which never prepares a split) identically, compares positions,
velocities, hash, index, cellStart, cellEnd and dens bit for bit after every call, and asserts nrs_resort_stats against the numbers
the build before nrs_host_state.h existed gives for the same sequence (each test was run on that build first; the full-sort context
never counts anything).  By the rule those numbers are: every full step behind a full step on the same arrays, grid and particle
count takes the queued split and counts 1; a partial step that ends at the hash or the sort drops the split uncounted; an upload, a
changed particle count or a changed grid drops it; no step fell back to the full sort (the mover share stays far below 50 %).
"""
import numpy as np
import pytest

from nereus_amd import capi
from tests.common import rel_err, small_dam_break
from tests.oracle_lib import SESPH, Oracle

pytestmark = pytest.mark.gpu

LATTICE = (34, 32, 32)
TOL_STEPS = 1e-5  # positions / velocities after N steps against the oracle (tests/test_parity_gpu.py)
_scene = {}


def scene_big():
    if not _scene:
        p, sc = small_dam_break(LATTICE)
        assert len(sc["pos"]) == 34 * 32 * 32 > 32768
        _scene["s"] = (p, sc)
    return _scene["s"]


def solver(flags, p, sc, bi=None, vbi=None):
    s = capi.Solver(p, len(sc["pos"]), flags=flags)
    s.set_particles(sc["pos"], sc["vel"])
    s.set_boundaries(sc["bi"] if bi is None else bi, sc["vbi"] if vbi is None else vbi, update_grid=True)
    return s


def pair():
    p, sc = scene_big()
    return solver(0, p, sc), solver(capi.FLAG_FULL_SORT, p, sc)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(d, f, what):
    """the two contexts hold the same bits"""
    for name in ("hash", "index", "cellStart", "cellEnd", "dens"):
        np.testing.assert_array_equal(bits(d.get(name)), bits(f.get(name)), err_msg="%s: %s" % (what, name))
    for name, a, b in zip(("pos", "vel"), d.download(), f.download()):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg="%s: %s" % (what, name))


def both(d, f, what, call):
    call(d)
    call(f)
    same(d, f, what)


def stats(d, f, what, want):
    got = d.resort_stats()
    print("%s: resort_stats %r (full-sort context %r)" % (what, got, f.resort_stats()))
    assert got == want, (what, got, want)
    assert f.resort_stats() == (0, 0), what


def reupload(s):
    pos, vel = s.download()
    s.set_particles(pos, vel)


@pytest.mark.parametrize("stage", [capi.STAGE_HASH, capi.STAGE_SORT], ids=["hash", "sort"])
def test_partial_step_with_a_split_queued(hip_lib, stage):
    d, f = pair()
    both(d, f, "step(3)", lambda s: s.step(3))
    stats(d, f, "step(3)", (2, 0))
    both(d, f, "step_partial", lambda s: s.step_partial(stage))  # the queued split is dropped, not counted
    stats(d, f, "step_partial", (2, 0))
    both(d, f, "re-upload", reupload)
    both(d, f, "step(3) after the re-upload", lambda s: s.step(3))
    stats(d, f, "step(3) after the re-upload", (4, 0))
    assert 0 <= d.get_stat(capi.STAT_MOVERS) <= d.n // 2 and f.get_stat(capi.STAT_MOVERS) == -1.0


def test_parameter_change_on_the_same_grid_keeps_the_split(hip_lib):
    d, f = pair()
    both(d, f, "step(3)", lambda s: s.step(3))

    def new_dt(s):
        q = s.params.copy()
        q["timestep"][0] *= 0.5
        s.set_params(q)

    both(d, f, "set_params", new_dt)
    both(d, f, "step(3) after set_params", lambda s: s.step(3))
    stats(d, f, "step(3), set_params, step(3)", (5, 0))


def test_changing_n_keeps_or_drops_the_split(hip_lib):
    d, f = pair()
    n = d.n
    both(d, f, "step(3)", lambda s: s.step(3))
    both(d, f, "set_n(n)", lambda s: s._chk(s.lib.nrs_set_num_particles(s.h, n)))  # the same count: the keys stay
    both(d, f, "step(2)", lambda s: s.step(2))
    stats(d, f, "step(3), set_n(n), step(2)", (4, 0))
    both(d, f, "set_n(n - 1000)", lambda s: s._chk(s.lib.nrs_set_num_particles(s.h, n - 1000)))  # another count: dropped
    both(d, f, "step(3)", lambda s: s.step(3))
    stats(d, f, "..., set_n(n - 1000), step(3)", (6, 0))
    assert d.n == f.n == n - 1000


def test_regrid_with_a_split_queued(hip_lib):
    """test_regrid_between_steps_invalidates_prepared_keys (tests/test_parity_gpu.py) at a size where the split of the old grid's
    keys is queued when the grid changes: shifted tank (new origin, same cell count), then a smaller tank (fewer cells)"""
    p, sc = scene_big()
    d, f = pair()
    o = Oracle(p, False, 1, SESPH, threads=8)
    o.set_particles(sc["pos"], sc["vel"])
    o.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    o.step(3)
    both(d, f, "step(3)", lambda s: s.step(3))
    np.testing.assert_array_equal(d.get("hash"), o.get("hash"))
    want = 2
    for variant in ("shifted", "smaller"):
        bi = sc["bi"].copy()
        if variant == "shifted":
            bi[:, :3] += np.array([0.013, 0.0, 0.071], dtype=bi.dtype)
            vbi = sc["vbi"]
        else:  # drop the far third of the tank in x: the AABB (and the pow2 grid) shrinks
            keep = bi[:, 0] <= 0.62 * bi[:, 0].max()
            bi, vbi = bi[keep], sc["vbi"][keep]
        o.set_boundaries(bi, vbi, update_grid=True)
        both(d, f, variant, lambda s: s.set_boundaries(bi, vbi, update_grid=True))
        np.testing.assert_array_equal(d.params.view(np.uint8), o.params.view(np.uint8))
        o.step(3)
        both(d, f, variant + ", step(3)", lambda s: s.step(3))
        want += 2
        stats(d, f, variant + ", step(3)", (want, 0))
        np.testing.assert_array_equal(d.get("hash"), o.get("hash"))
        np.testing.assert_array_equal(d.get("index"), o.get("index"))
        gp, gv = d.download()
        assert rel_err(gp[:, :3], o.get("pos")[:, :3]) <= TOL_STEPS
        assert rel_err(gv[:, :3], o.get("vel")[:, :3]) <= TOL_STEPS


def test_density_stop_then_upload_then_full_steps(hip_lib):
    """a step that ends at the density stage: its plan shares no hit lists and prepares no keys, its sort takes the queued split"""
    d, f = pair()
    both(d, f, "step(3)", lambda s: s.step(3))
    both(d, f, "step_partial(DENSITY)", lambda s: s.step_partial(capi.STAGE_DENSITY))
    stats(d, f, "step(3), step_partial(DENSITY)", (3, 0))
    both(d, f, "re-upload", reupload)
    both(d, f, "step(3) after the re-upload", lambda s: s.step(3))
    stats(d, f, "step(3) after the re-upload", (5, 0))
