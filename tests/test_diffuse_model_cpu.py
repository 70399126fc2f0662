"""The numpy model of the diffuse particles (tests/diffuse_model.py) on hand cases, and the settings of the GPU tests
(tests/test_diffuse_gpu.py): on the golden dam break the model alone must produce every kind of particle, hit the per-particle cap and
overflow half its own total, so that the device tests cannot pass vacuously.
"""
import os

import numpy as np
import pytest

from nereus_amd.params import default_params
from tests import diffuse_model as dm
from tests import pcisph_model as pm
from tests.common import small_dam_break

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The settings of the GPU tests.  The scene has 4 to 10 neighbours per particle (spacing 0.04, h 0.0457), |v| up to 0.5: the clamp ranges
# bracket the potentials the model finds there, the rates turn a potential of 1 into a few births per step of 1 ms.
SETTINGS = dict(seed=2012, tau_ta=(0.1, 0.5), tau_wc=(0.1, 1.0), tau_k=(5e-4, 4e-3), k_ta=3000.0, k_wc=3000.0, lifetime=(0.002, 0.02),
                k_buoyancy=2.0, k_drag=0.5, spray_below=5, bubble_above=6, max_per_particle=3)
STEPS = 10


def golden_state():
    """(params, pos, vel): the golden SESPH dam break after ten steps with the random velocities of the GPU tests' dam state"""
    d = np.load(os.path.join(ROOT, "tests", "golden", "sesph_dambreak.npz"))
    p, _ = small_dam_break((12, 10, 9))
    params = np.frombuffer(d["params"].tobytes(), dtype=p.dtype).copy()
    pos = d["pos10"].copy()
    vel = np.zeros_like(pos)
    vel[:, :3] = np.random.default_rng(11).uniform(-0.3, 0.3, (len(pos), 3))
    return params, pos, vel


def run_model(params, pos, vel, cfg, steps=STEPS, capacity=None, kernel_set=pm.MULLER):
    """`steps` diffuse steps of the model on one fluid state from an empty set: the list of step() results"""
    real = pm.real_of(params)
    dpos, dvel = np.zeros((0, 4), real), np.zeros((0, 4), real)
    out = []
    for k in range(steps):
        r = dm.step(params, cfg, pos, vel, dpos, dvel, k, 0.0, kernel_set, capacity)
        dpos, dvel = r["pos"], r["vel"]
        out.append(r)
    return out


_unbounded = {}


def unbounded():
    if "r" not in _unbounded:
        params, pos, vel = golden_state()
        _unbounded["r"] = run_model(params, pos, vel, dm.config(capacity=1 << 20, **SETTINGS))
    return _unbounded["r"]


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------------
def pair_params(double=False):
    p = default_params(0, double)
    p["gridSize"][0] = (8, 8, 8)
    p["numCells"][0] = 512
    p["worldOrigin"][0] = (0.0, 0.0, 0.0)
    p["cellSize"][0] = (p["interactionRadius"][0],) * 3
    return p


@pytest.mark.parametrize("double", [False, True])
def test_two_particles_closing_and_receding(double):
    p = pair_params(double)
    real = pm.real_of(p)
    h = float(p["interactionRadius"][0])
    pos = np.ones((2, 4), real)
    pos[:, :3] = [(3.3 * h, 3.5 * h, 3.5 * h), (3.8 * h, 3.5 * h, 3.5 * h)]
    vel = np.zeros((2, 4), real)
    vel[:, 0] = (0.25, -0.5)  # closing head-on along x: |v_ij| = 0.75
    F = dm.fluid_pass(p, dm.config(), pos, vel, 0, 1e-3, raw=True)
    want = 2 * 0.75 * 0.5
    assert np.allclose(F["ta"], want, rtol=1e-5), F["ta"]
    vel[:, 0] = (-0.25, 0.5)  # receding
    F = dm.fluid_pass(p, dm.config(), pos, vel, 0, 1e-3, raw=True)
    assert np.all(F["ta"] == 0), F["ta"]


def test_lone_moving_particle_has_only_kinetic_energy():
    p = pair_params()
    h = float(p["interactionRadius"][0])
    pos = np.array([[2.5 * h, 2.5 * h, 2.5 * h, 1.0]], np.float32)
    vel = np.array([[0.3, -0.4, 1.2, 0.0]], np.float32)
    F = dm.fluid_pass(p, dm.config(), pos, vel, 0, 1e-3, raw=True)
    assert F["ta"][0] == 0 and F["wc"][0] == 0 and not F["normals"].any()
    assert np.isclose(F["ek"][0], 0.5 * float(p["particleMass"][0]) * (0.09 + 0.16 + 1.44), rtol=1e-6)
    assert F["potentials"][0, 0] == 0 and F["potentials"][0, 1] == 0 and F["births"][0] == 0 and F["count"][0] == 1


def test_uniform_stream():
    step, slot, draw = np.meshgrid(np.arange(12), np.arange(3000), np.arange(41), indexing="ij")
    hh = dm.hash64(2012, step.ravel(), slot.ravel(), draw.ravel())
    assert len(np.unique(hh)) == hh.size  # no repeats across (step, slot, draw)
    assert len(np.unique(np.concatenate((hh, dm.hash64(2013, step.ravel(), slot.ravel(), draw.ravel()))))) == 2 * hh.size
    for real in (np.float32, np.float64):
        u = dm.uniform(2012, step.ravel(), slot.ravel(), draw.ravel(), real)
        assert u.dtype == real and u.min() >= 0 and u.max() < 1
        # n = 1.476 M draws: the mean of a uniform has standard deviation 1 / sqrt(12 n) = 2.4e-4; five of them
        assert abs(float(u.astype(np.float64).mean()) - 0.5) < 5 / np.sqrt(12 * u.size)
        assert np.all(u.astype(np.float64) * 2.0 ** 24 == np.floor(u.astype(np.float64) * 2.0 ** 24))  # 24-bit fractions, exact
        # each of 16 equal bins holds n / 16 within five standard deviations of a binomial
        c = np.bincount((u.astype(np.float64) * 16).astype(int), minlength=16)
        assert np.abs(c - u.size / 16).max() < 5 * np.sqrt(u.size * (1 / 16) * (15 / 16))


def test_disc_rule():
    rng = np.random.default_rng(1)
    for real in (np.float32, np.float64):
        ua, ub = rng.uniform(-1, 1, (5000, 4)).astype(real), rng.uniform(-1, 1, (5000, 4)).astype(real)
        ua[:7], ub[:7] = 0.9, 0.9  # no pair inside: the centre
        ua[7, :3], ub[7, :3], ua[7, 3], ub[7, 3] = 0.9, 0.9, 0.25, -0.5  # the last pair wins
        a, b = dm.disc_point(ua, ub, real)
        assert np.all(a * a + b * b < 1)
        assert not a[:7].any() and not b[:7].any() and (a[7], b[7]) == (0.25, -0.5)
        first = ua[:, 0] ** 2 + ub[:, 0] ** 2 < 1
        assert np.all(a[first] == ua[first, 0]) and np.all(b[first] == ub[first, 0])


def test_frame_is_orthonormal():
    rng = np.random.default_rng(2)
    v = rng.normal(size=(500, 3))
    v[0] = (0, 0, 0)
    v[1] = (0, 2, 0)
    v[2] = (1, 1, 1)
    e1, e2 = dm.frame(v, np.float64)
    assert np.all(e1[0] == (1, 0, 0)) and np.all(e2[0] == (0, 1, 0))
    vh = v[1:] / np.linalg.norm(v[1:], axis=1)[:, None]
    for a, b in ((e1[1:], e1[1:]), (e2[1:], e2[1:])):
        assert np.allclose((a * b).sum(1), 1, atol=1e-6)
    for a, b in ((e1[1:], e2[1:]), (e1[1:], vh), (e2[1:], vh)):
        assert np.abs((a * b).sum(1)).max() < 1e-6


# ---- the settings of the GPU tests are not vacuous ---------------------------------------------------------------------------------------------
def test_settings_produce_every_kind_hit_the_cap_and_overflow():
    runs = unbounded()
    seen = np.zeros(3, np.int64)
    for r in runs:
        seen = np.maximum(seen, r["by_kind"])
    print("largest count per kind within %d steps: %s; final total %d" % (STEPS, seen, runs[-1]["alive"]))
    assert seen.min() >= 50, seen
    assert any((r["births"] == SETTINGS["max_per_particle"]).any() for r in runs)
    assert any(r["survivors"] < before["alive"] for before, r in zip(runs, runs[1:]))  # (some die, too)
    total = runs[-1]["alive"]
    params, pos, vel = golden_state()
    cap = total // 2
    small = run_model(params, pos, vel, dm.config(capacity=cap, **SETTINGS))
    assert sum(r["dropped"] for r in small) > 0 and max(r["alive"] for r in small) == cap
    # up to the first overflow both runs are the same
    first = next(k for k, r in enumerate(small) if r["dropped"])
    assert first >= 1
    assert small[first]["pos"].tobytes() == runs[first]["pos"][:cap].tobytes()
    assert small[first]["dropped"] == runs[first]["total"] - cap
