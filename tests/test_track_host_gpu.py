"""Particle tracking through the C++ host classes (Nereus::SPH::setParticleTracking, getHostIds / getHostBirth / getHostCol,
setEmitterColor, diffuseColors, locateParticles in nereus_amd/host) driven by the headless driver's `track` and `colours` modes."""
import subprocess

import numpy as np
import pytest

from tests.test_host_class import _driver

pytestmark = pytest.mark.gpu

STEPS = 60
RED, BLUE = (1.0, 0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1.0)


def run_track(tmp_path, kind, kappa):
    out = str(tmp_path / ("track_%s_%g.txt" % (kind, kappa)))
    subprocess.check_call([_driver(), "track", kind, str(STEPS), out, repr(kappa)], stdout=subprocess.DEVNULL)
    a = np.loadtxt(out, ndmin=2)
    return a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), a[:, 2:5], a[:, 5:9]


@pytest.mark.parametrize("kind", ["sesph", "dfsph"])
def test_headless_track(tmp_path, hip_lib, kind):
    ids, birth, pos, col = run_track(tmp_path, kind, 0.0)
    n = len(ids)
    assert n > 200 and len(np.unique(ids)) == n  # every id occurs once
    red, blue = (col == RED).all(axis=1), (col == BLUE).all(axis=1)
    assert np.all(red | blue) and red.sum() > 50 and blue.sum() > 50  # before the first diffuseColors: one of the two emitters' colours
    assert np.all(pos[red, 0] < 0) and np.all(pos[blue, 0] > 0)        # ... and the colour of the jet the particle is in
    for mask in (red, blue):  # births are non-decreasing in id within each emitter
        o = np.argsort(ids[mask])
        assert np.all(np.diff(birth[mask][o]) >= 0) and len(set(birth[mask].tolist())) >= 3
    assert birth.max() < STEPS
    # with diffusion the same particles, colours between the two emitters'
    ids2, birth2, pos2, col2 = run_track(tmp_path, kind, 0.05)
    assert sorted(ids2.tolist()) == sorted(ids.tolist()) and len(np.unique(ids2)) == len(ids2)
    lo, hi = np.minimum(RED, BLUE), np.maximum(RED, BLUE)
    assert np.all(col2 >= lo - 1e-6) and np.all(col2 <= hi + 1e-6)
    assert np.all(col2[:, 1] == 0) and np.all(col2[:, 3] == 1)       # (a constant channel, and the channel with kappa 0)
    mixed = (col2[:, 0] > 0.01) & (col2[:, 0] < 0.99)
    assert mixed.sum() > 20                                            # the jets touch: colour has crossed
    assert abs(float((col2[:, 0] + col2[:, 2]).mean()) - 1.0) < 1e-4  # red + blue stays 1 per particle (the same weights on both)


def test_colours_follow_their_particles(tmp_path, hip_lib):
    def run(track):
        out = str(tmp_path / ("colours_%d.txt" % track))
        subprocess.check_call([_driver(), "colours", "sesph", "5", str(track), out], stdout=subprocess.DEVNULL)
        return np.loadtxt(out, ndmin=2)
    a = run(1)
    k, slot, ident, r = a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), a[:, 2].astype(np.int64), a[:, 3]
    n = len(k)
    assert n == 2197 and sorted(slot.tolist()) == list(range(n)) and slot.tolist() != list(range(n))  # the steps did permute
    assert np.array_equal(ident, k) and np.array_equal(r, k.astype(np.float64))  # the colour written for particle k is at locateParticles(k, 1)
    b = run(0)
    assert np.array_equal(b[:, 1], b[:, 0]) and np.array_equal(b[:, 3], b[:, 0])  # without tracking getHostCol() is as it was filled
