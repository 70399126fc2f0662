"""Hand cases of the sources' and sinks' numpy model (tests/inflow_model.py; include/nereus_hip.h "sources and sinks"): the schedule, the
frame, the site counts, the capacity and max_particles rules, the predicate's edges and the compaction; and that the scenes the GPU
tests use (tests/test_inflow_gpu.py) are not vacuous.  No GPU.
"""
import numpy as np
import pytest

from tests import inflow_model as im
from tests.common import small_dam_break

# exact binary values: speed * dt = s / 4 without a rounding
S, DT, SPEED = 1.0 / 32.0, 1.0 / 1024.0, 8.0
DT_TWO = 2.3 * S / SPEED  # one step of it yields two layers
FAUCET = dict(center=(0.4, 0.4, 0.23), direction=(0.0, -2.0, 0.0), half_extent=2.5 * S, speed=SPEED, spacing=S, shape=im.DISC)
LOCKSTEP_STEPS = 24


def sink_scene(double=False, ks=1, solver=0):
    """small_dam_break with one particle outside the grid, and a box over the top two lattice layers of the column"""
    p, sc = small_dam_break((12, 10, 9), double=double, kernel_set=ks, solver=solver)
    real = np.float64 if double else np.float32
    d = float(real(p["interactionRadius"][0])) - 0.005  # the lattice spacing of scene.fluid_block
    pos = np.concatenate([sc["pos"], np.array([[40.0, 0.3, 0.2, 1.0]], real)])
    vel = np.zeros_like(pos)
    box = [-1.0, 8.5 * d, -1.0, 3.0, 12.0 * d, 3.0]
    return p, sc, pos, vel, box


def params():
    return small_dam_break()[0]


def test_quarter_spacing_gives_a_layer_every_fourth_step():
    e = im.Emitter(params(), speed=SPEED, **{k: v for k, v in FAUCET.items() if k != "speed"})
    got = [e.schedule(DT, 10 ** 9) for _ in range(12)]
    assert [len(g) for g in got] == [0, 0, 0, 1] * 3
    assert all(g == [0.0] for g in got[3::4])  # the accumulator is spent exactly: the layer's origin is the centre
    pos, vel = e.layer(0.0, np.float32)
    assert np.array_equal(pos[10, :3], np.array(FAUCET["center"], np.float32))  # site (0, 0) is the middle one of 21
    assert np.array_equal(vel[0], np.array([0.0, -8.0, 0.0, 0.0], np.float32)) and np.all(pos[:, 3] == 1.0)
    assert np.all(pos[:, 1] == np.float32(0.4))  # the layer is normal to d


def test_two_layers_in_one_step():
    e = im.Emitter(params(), **FAUCET)
    offs = e.schedule(DT_TWO, 10 ** 9)
    assert len(offs) == 2 and offs[0] == pytest.approx(1.3 * S, rel=1e-12) and offs[1] == pytest.approx(0.3 * S, rel=1e-12)
    o = np.array(FAUCET["center"]) + offs[0] * np.array([0.0, -1.0, 0.0])
    pos, _ = e.layer(offs[0], np.float64)
    assert np.array_equal(pos[10, :3], o)
    assert e.acc == offs[1] and e.emitted == 42


def test_site_counts():
    assert len(im.sites(im.DISC, (2.5 * S, 0.0), S)) == 21
    assert len(im.sites(im.DISC, (0.0, 0.0), S)) == 1
    for hu, hv, ku, kv in ((3.2 * S, 1.0 * S, 3, 1), (0.0, 2.9 * S, 0, 2), (0.99 * S, 0.99 * S, 0, 0)):
        ij = im.sites(im.RECT, (hu, hv), S)
        assert len(ij) == (2 * ku + 1) * (2 * kv + 1)
        assert ij[0].tolist() == [-ku, -kv] and ij[-1].tolist() == [ku, kv]
        if ku:
            assert ij[1].tolist() == [-ku + 1, -kv]  # j-major: i runs fastest
    d = im.sites(im.DISC, (2.5 * S, 0.0), S)
    assert d[0].tolist() == [-1, -2] and d[-1].tolist() == [1, 2] and d[10].tolist() == [0, 0]


def test_spacing_default_is_the_rest_spacing():
    p = params()
    assert im.spacing_of(0.0, p) == pytest.approx((float(p["particleMass"][0]) / float(p["restDensity"][0])) ** (1.0 / 3.0), rel=1e-15)
    assert im.spacing_of(0.25, p) == 0.25


@pytest.mark.parametrize("d,e1,e2", [
    ((1, 0, 0), (0, 0, 1), (0, -1, 0)),    # tie between y and z: the lowest, y, is the axis; x cross y = z, x cross z = -y
    ((0, 1, 0), (0, 0, -1), (-1, 0, 0)),   # tie between x and z: x; y cross x = -z, y cross -z = -x
    ((0, 0, 1), (0, 1, 0), (-1, 0, 0)),    # tie between x and y: x; z cross x = y, z cross y = -x
    ((0, -3, 0), (0, 0, 1), (-1, 0, 0)),   # normalised first; -y cross x = z, -y cross z = -x
])
def test_frame_along_the_axes(d, e1, e2):
    fd, f1, f2 = im.frame(d)
    assert np.array_equal(fd, np.array(d, np.float64) / np.abs(d).max())
    assert np.array_equal(f1, np.array(e1, np.float64)) and np.array_equal(f2, np.array(e2, np.float64))


def test_frame_tie_and_orthonormal():
    fd, f1, f2 = im.frame((1.0, 1.0, 1.0))  # a three-way tie: x is the axis
    want = im.cross(fd, np.array([1.0, 0.0, 0.0]))
    assert np.array_equal(f1, want / im.length(want))
    for d in ((1.0, 1.0, 1.0), (0.3, -0.2, 0.9), (-5.0, 0.1, 0.1)):
        fd, f1, f2 = im.frame(d)
        m = np.stack([fd, f1, f2])
        assert np.allclose(m @ m.T, np.eye(3), atol=1e-15)
        assert np.allclose(np.cross(fd, f1), f2, atol=1e-15)


def test_capacity_drops_whole_layers_without_a_burst():
    e = im.Emitter(params(), **FAUCET)
    room = 50  # two layers of 21 fit, the third does not
    sizes = []
    for _ in range(16):
        offs = e.schedule(DT, room)
        room -= 21 * len(offs)
        sizes.append(len(offs))
    assert sizes == [0, 0, 0, 1, 0, 0, 0, 1] + [0] * 8
    assert e.emitted == 42 and e.dropped == 42 and room == 8
    assert e.acc == 0.0  # the accumulator went on: room later does not release a burst
    assert e.schedule(DT, 10 ** 6) == [] and e.emitted == 42


def test_max_particles():
    e = im.Emitter(params(), max_particles=50, **FAUCET)
    for _ in range(16):
        e.schedule(DT, 10 ** 9)
    assert e.emitted == 42 and e.dropped == 42
    e = im.Emitter(params(), max_particles=42, **FAUCET)
    assert len(e.schedule(DT_TWO, 10 ** 9)) == 2 and e.dropped == 0
    off = im.Emitter(params(), enabled=False, **FAUCET)
    assert off.schedule(DT_TWO, 10 ** 9) == [] and off.acc == 0.0


@pytest.mark.parametrize("real", [np.float32, np.float64])
def test_predicate_edges(real):
    p = params()
    box = [0.25, 0.5, 0.75, 0.5, 1.0, 1.5]
    lo, hi = im.domain(p, real)
    inside = [0.3, 0.6, 0.8, 1.0]
    rows = [inside, [0.25, 0.5, 0.75, 1.0], [0.5, 0.6, 0.8, 1.0], [0.3, 1.0, 0.8, 1.0], [0.3, 0.6, 1.5, 1.0],
            [np.nextafter(real(0.5), real(0)), np.nextafter(real(1.0), real(0)), np.nextafter(real(1.5), real(0)), 1.0],
            [np.nextafter(real(0.25), real(0)), 0.6, 0.8, 1.0]]
    got = im.caught(p, np.array(rows, real), real, boxes=[box])
    assert got.tolist() == [True, True, False, False, False, True, False]  # min inclusive, max exclusive
    bad = np.array([[np.nan, 0, 0, 1], [0, np.inf, 0, 1], [0, 0, -np.inf, 1], [0, 0, 0, np.nan], [0, 0, 0, 1]], real)
    assert im.caught(p, bad, real).tolist() == [True, True, True, False, False]  # w is not a coordinate
    edge = np.array([[lo[0], lo[1], lo[2], 1], [hi[0], 0, 0, 1], [np.nextafter(hi[0], real(0)), 0, 0, 1], [0, np.nextafter(lo[1], real(-9)), 0, 1],
                     [0, 0, hi[2], 1]], real)
    assert im.caught(p, edge, real, domain_on=True).tolist() == [False, True, False, True, True]
    assert not im.caught(p, edge, real).any()  # without NRS_SINK_DOMAIN the grid box does not matter
    assert hi.dtype == real and lo.dtype == real


def test_compaction_keeps_order_and_moves_arrays_together():
    gone = np.array([True, False, False, True, False])
    a, b, c = im.compact(gone, np.arange(5), np.arange(5) * 10.0, None)
    assert a.tolist() == [1, 2, 4] and b.tolist() == [10.0, 20.0, 40.0] and c is None
    assert [im.cull_due(k, 3) for k in range(1, 8)] == [False, False, True, False, False, True, False]
    assert all(im.cull_due(k, 0) and im.cull_due(k, 1) for k in range(1, 5))


def test_block_order_and_positions():
    pos, vel = im.block((0.1, 0.2, 0.3), (0.5, 0.25, 0.125), (3, 2, 2), (1.0, 2.0, 3.0), np.float32)
    assert len(pos) == 12
    assert pos[1, :3].tolist() == [np.float32(0.1 + 0.5), np.float32(0.2), np.float32(0.3)]  # i runs fastest
    assert pos[3, :3].tolist() == [np.float32(0.1), np.float32(0.2 + 0.25), np.float32(0.3)]
    assert pos[6, :3].tolist() == [np.float32(0.1), np.float32(0.2), np.float32(0.3 + 0.125)]
    assert np.all(vel == np.array([1, 2, 3, 0], np.float32)) and np.all(pos[:, 3] == 1)


def test_sink_scene_is_not_vacuous():
    """from the uploaded scene alone: the box removes particles in at least three different 256-slot groups and keeps most; the domain
    catches the one particle outside the grid and nothing else"""
    for double in (False, True):
        real = np.float64 if double else np.float32
        p, sc, pos, vel, box = sink_scene(double)
        # (the grid the context uses comes from the boundary box; the default grid of p is larger, 40 m lies outside both)
        by_box = im.caught(p, pos, real, boxes=[box])
        by_domain = im.caught(p, pos, real, domain_on=True)
        assert by_domain.sum() == 1 and by_domain[-1] and not by_box[-1]
        assert by_box.sum() == 12 * 2 * 9
        groups = np.unique(np.nonzero(by_box)[0] // 256)
        assert len(groups) >= 3
        assert (by_box | by_domain).sum() < 0.25 * len(pos)


def test_lockstep_schedule_is_not_vacuous():
    """the schedule of the emitter lockstep test: two layers in the first step (dt = DT_TWO), then a layer every fourth step"""
    e = im.Emitter(params(), **FAUCET)
    counts = [len(e.schedule(DT_TWO if k == 0 else DT, 10 ** 9)) for k in range(LOCKSTEP_STEPS)]
    assert counts[0] == 2 and sum(1 for c in counts if c) >= 6 and max(counts[1:]) == 1
    assert e.emitted == 21 * sum(counts)
