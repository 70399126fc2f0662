"""The read-out side on random scenes (tools/fuzz_parity.py one_sample, one_surface, one_aniso, one_diffuse, one_track_diffuse): the
field sampler, the surface mesher, the anisotropic passes, the diffuse-particle step and the attribute diffusion on unscaled pieces of
the soak's scenes — cells of 1.25 h x 1.4 h x h, grids with a four-cell axis, clouds that wrap through the grid, origins thousands of
cells away, clumps with more than 128 particles in a cell, wall sheets, NaN / inf particles, fp32 and fp64, both kernel sets by seed —
against the models of tests/, with the bars of the readers' own test files.  One case per reader and seed: one small context and one
model run.  tests/test_readers_fuzz_cpu.py shows, without a device, that the slice holds every class, that the models' brute-force
pairs are the walk's, that their runs are not vacuous and that the comparisons notice a mutated model.

Every case prints its figures and records them in readers_fuzz.json, next to the drift record of tests/test_fast_arith_gpu.py
(record_drift); DESIGN.md "Field sampling" quotes the maxima.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

SEEDS = range(9400, 9424)


def run(reader, seed):
    import fuzz_parity as fp
    from tests.test_fast_arith_gpu import record_drift

    errors = {}
    r = fp.READERS[reader](seed, errors)
    print("%s %d: %s" % (reader, seed, errors.get(seed)))
    if seed in errors:
        record_drift("%s %d" % (reader, seed), 0, None, None, file="readers_fuzz.json", entry=errors[seed])
    assert r is None, r
    assert seed in errors


@pytest.mark.parametrize("seed", SEEDS)
def test_sampler(hip_lib, seed):
    """nrs_sample_points on about 700 queries (particle positions, points whose cells wrap, +-1e30, NaN, inf, points next to walls)
    without and with the wall term: counts exact, error / bound <= 1; nrs_sample_lattice byte-equal to the points call on its nodes"""
    run("sample", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_surface(hip_lib, seed):
    """nrs_surface_extract at 0.5 rho0 with both attributes: bit for bit the model's mesh on the sampler's arrays, closed unless the
    wall term reaches the lattice border.  Even seeds set SURFACE_WALLS; it changes the meshed density on 9416 and 9422, the scenes
    whose wall sheet reaches the lattice (there it must, and away from the walls it must not)"""
    run("surface", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_aniso(hip_lib, seed):
    """pass A: count, index and liveness exact, centre / weight / bound / G within RECORD_CAP; the extract bit for bit the model's on
    the sampled phi; pass B within the model's a-priori bound of the device's own records"""
    run("aniso", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_diffuse(hip_lib, seed):
    """three nrs_diffuse_steps in lockstep with the model, byte for byte, the fluid moved by upload; odd seeds at half the capacity"""
    run("diffuse", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_track_diffuse(hip_lib, seed):
    """two nrs_track_diffuse calls byte for byte against the model, walls included; the kappa = 0 channel unchanged"""
    run("track", seed)
