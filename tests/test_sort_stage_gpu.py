"""The two decisions of the sort stage (nrs_sort.h: SortStage::sort_keys, nrs_host_state.h: choose_sort) that no other single-domain
test reaches: a step whose queued split holds no mover (SortKind::MERGE_STAYERS: the stayers are the sorted sequence, no mover sort, no
merge) and a step whose split holds more than RESORT_MAX_MOVER_PCT = 50 % movers (the full radix sort, counted as a fallback).

The pattern of tests/test_call_sequences_gpu.py: fp32 Muller SESPH on small_dam_break((34, 32, 32)) with its walls, 34,816 particles
(RESORT_MIN_PARTICLES is 32,768); a default context and an NRS_FLAG_FULL_SORT context driven identically; positions, velocities, hash,
index, the cell tables and dens compared bit for bit after every call, hash and index also with the oracle.  What each test supposes
about the input - how many particles change cell in a step - is counted on the oracle's states on the CPU and asserted before the
device is looked at.  The nrs_resort_stats tuples and NRS_STAT_MOVERS values asserted are those the build before SortStage existed gives
for the same calls (each test was run on that build first); the mover counts are also the oracle's own counts, because the keys equal
the oracle's bit for bit.
"""
import numpy as np
import pytest

from nereus_amd import capi
from tests.common import small_dam_break
from tests.oracle_lib import SESPH, Oracle
from tests.test_call_sequences_gpu import LATTICE, same, solver

pytestmark = pytest.mark.gpu


def oracle_states(p, sc, steps):
    """(hash, index) of the oracle after each of `steps` steps, and per step after the first the number of particles whose cell
    differs from the one they were sorted into one step earlier: index[i] is the slot particle i of the new order had in the old"""
    o = Oracle(p, False, 1, SESPH, threads=8)
    o.set_particles(sc["pos"], sc["vel"])
    o.set_boundaries(sc["bi"], sc["vbi"], update_grid=True)
    states, changed = [], []
    for _ in range(steps):
        o.step(1)
        h, i = o.get("hash").copy(), o.get("index").copy()
        if states:
            changed.append(int((h != states[-1][0][i]).sum()))
        states.append((h, i))
    return states, changed


def step_and_compare(d, f, state, what):
    """one step on both contexts: the same bits on both, the oracle's keys and values"""
    d.step(1)
    f.step(1)
    same(d, f, what)
    np.testing.assert_array_equal(d.get("hash"), state[0], err_msg=what + ": hash against the oracle")
    np.testing.assert_array_equal(d.get("index"), state[1], err_msg=what + ": index against the oracle")
    got = d.resort_stats(), d.get_stat(capi.STAT_MOVERS)
    print("%s: resort_stats %r, movers %r" % (what, got[0], got[1]))
    assert f.resort_stats() == (0, 0) and f.get_stat(capi.STAT_MOVERS) == -1.0, what
    return got


def test_no_mover_takes_the_stayers_alone(hip_lib):
    """An unjittered lattice at rest, moved off the cell faces: along every axis the lattice planes (spacing h - 0.005) stand at least
    1.7 mm from a face of the 45.7 mm cells (the shift below is the best of 400 tried per axis), and a step under gravity moves a
    particle by less than 0.06 mm.  No particle changes cell during the first or the second step, so the second and the third step
    find a split without movers: counted as steps, no fallback, NRS_STAT_MOVERS 0."""
    p, sc = small_dam_break(LATTICE, jitter=0.0)
    sc = dict(sc)
    sc["pos"] = sc["pos"].copy()
    sc["pos"][:, :3] = (sc["pos"][:, :3].astype(np.float64) + np.array([0.02822, 0.02319, 0.02319])).astype(np.float32)
    states, changed = oracle_states(p, sc, 3)
    assert changed == [0, 0], changed  # the precondition, on the CPU
    d, f = solver(0, p, sc), solver(capi.FLAG_FULL_SORT, p, sc)
    assert step_and_compare(d, f, states[0], "step 1") == ((0, 0), -1.0)  # hashed and sorted in full: no split was queued
    assert step_and_compare(d, f, states[1], "step 2") == ((1, 0), 0.0)
    assert step_and_compare(d, f, states[2], "step 3") == ((2, 0), 0.0)


def test_most_particles_move_falls_back_to_the_full_sort(hip_lib):
    """Every particle at (20, 12, 8) m/s, away from the walls: 20, 12 and 8 mm per step across 45.7 mm cells.  On the oracle 71.7 % of
    the particles change cell during the first step (asserted: between 55 % and 90 %), 62.1 % during the second: above
    RESORT_MAX_MOVER_PCT both times, so the second and the third step each count a step and a fallback and sort in full."""
    p, sc = small_dam_break(LATTICE)
    sc = dict(sc)
    sc["vel"] = sc["vel"].copy()
    sc["vel"][:, :3] = np.array([20.0, 12.0, 8.0], np.float32)
    n = len(sc["pos"])
    states, changed = oracle_states(p, sc, 3)
    print("cell changers per step on the oracle: %r of %d" % (changed, n))
    assert 0.55 * n <= changed[0] <= 0.90 * n, (changed, n)  # the precondition, on the CPU
    d, f = solver(0, p, sc), solver(capi.FLAG_FULL_SORT, p, sc)
    assert step_and_compare(d, f, states[0], "step 1") == ((0, 0), -1.0)
    assert step_and_compare(d, f, states[1], "step 2") == ((1, 1), float(changed[0]))
    # the third step: what the build before SortStage does - the second step's changers are again more than half
    assert 2 * changed[1] > n, (changed, n)
    assert step_and_compare(d, f, states[2], "step 3") == ((2, 2), float(changed[1]))
