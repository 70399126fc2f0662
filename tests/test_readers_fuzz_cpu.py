"""The scenes and the models of tests/test_readers_fuzz_gpu.py, without a device (tools/fuzz_parity.py make_reader_scene, one_sample ..
one_track_diffuse): the slice of seeds must hold every class of geometry the readers can go wrong on, the models' brute-force pairs
must be the pairs the device's cell walk meets (no pair dropped), the models' own runs must not be vacuous (every tetrahedron case,
every kind of diffuse particle, deaths, the birth cap, a capacity that overflows), and a model mutated in one place must fail the
comparison the GPU tests make — so a device wrong in that place would.
"""
import os
import sys

import numpy as np
import pytest

from tests import diffuse_model as dm
from tests import sample_model as spm
from tests import surface_model as sfm
from tests import track_model as tm
from tests.test_track_model_cpu import KAPPA, record_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_parity as fp  # noqa: E402

SEEDS = range(9400, 9424)
_scenes, _runs, _dens = {}, {}, {}


def scene(seed):
    if seed not in _scenes:
        _scenes[seed] = fp.make_reader_scene(seed)
    return _scenes[seed]


def diffuse_run(seed):
    if seed not in _runs:
        _runs[seed] = fp.reader_diffuse_run(scene(seed))
    return _runs[seed]


def finite(sc):
    return sc["pos"][np.all(np.isfinite(sc["pos"]), axis=1)]


def cell_counts(sc):
    g = np.array(sc["gs"])
    c = dm.cells(sc["p"], finite(sc), sc["real"]) & (g - 1)
    return np.bincount(np.unique((c[:, 2] * g[1] + c[:, 1]) * g[0] + c[:, 0], return_inverse=True)[1])


# ---- 1. the scenes ----------------------------------------------------------------------------------------------------------------------------
def test_existing_scenes_keep_their_draws():
    """make_reader_scene draws from a generator of its own: make_scene and make_model_scene give what they gave"""
    a = fp.make_scene(9404)
    fp.make_reader_scene(9404)
    b = fp.make_scene(9404)
    assert a["pos"].tobytes() == b["pos"].tobytes() and a["vel"].tobytes() == b["vel"].tobytes() and a["gs"] == b["gs"]
    assert a["p"].tobytes() == b["p"].tobytes()
    assert fp.make_reader_scene(9404)["pos"].tobytes() == fp.make_reader_scene(9404)["pos"].tobytes()


def test_the_slice_holds_every_class():
    c = dict(fp64=0, monaghan=0, far=0, outside=0, wide_cell=0, four_cells=0, walls=0, nonfinite=0, over64=0, over128=0)
    for sd in SEEDS:
        sc = scene(sd)
        p, h = sc["p"], sc["h"]
        assert 300 <= sc["n"] - sc["nonfinite"] <= 1500 and (sc["bi"] is None or len(sc["bi"]) <= 1500)
        assert np.all(np.asarray(p["cellSize"][0]) >= p["interactionRadius"][0]) and min(sc["gs"]) >= 4
        assert all(g & (g - 1) == 0 for g in sc["gs"]) and np.abs(sc["vel"][:, :3]).max() > 0
        lo = np.asarray(p["worldOrigin"][0], np.float64)
        hi = lo + np.array(sc["gs"]) * np.asarray(p["cellSize"][0], np.float64)
        x = finite(sc)[:, :3]
        cc = cell_counts(sc)
        c["fp64"] += sc["double"]
        c["monaghan"] += sc["kset"] == 0
        c["far"] += bool(np.abs((x[0] - lo) / np.asarray(p["cellSize"][0], np.float64)).max() > 4096)
        c["outside"] += bool(np.any((x < lo) | (x >= hi)))
        c["wide_cell"] += bool(np.any(sc["cs"] > h))
        c["four_cells"] += min(sc["gs"]) == 4
        c["walls"] += sc["bi"] is not None
        c["nonfinite"] += sc["nonfinite"] > 0
        c["over64"] += cc.max() > 64
        c["over128"] += cc.max() > 128
    print(c)
    need = dict(fp64=3, monaghan=6, far=2, outside=5, wide_cell=8, four_cells=1, walls=10, nonfinite=1, over64=3, over128=1)
    assert all(c[k] >= v for k, v in need.items()), c
    assert scene(9400)["double"] and not scene(9417)["double"]  # (a far origin in each precision)
    sc = scene(9404)  # the NaN / inf rows sit behind the piece, with their velocities
    assert sc["nonfinite"] >= 3 and not np.isfinite(sc["pos"][-sc["nonfinite"]:, :3]).all(axis=1).any() and np.isfinite(sc["pos"][:-sc["nonfinite"]]).all()
    assert fp.make_reader_scene(9404, min_axis=8, max_particles=400)["n"] == 400 and min(fp.make_reader_scene(9411, min_axis=8)["gs"]) == 8


# ---- 2. the candidate rule -----------------------------------------------------------------------------------------------------------------
def test_dropped_pairs_counts_what_the_walk_misses():
    sc = scene(9405)
    x = finite(sc)
    assert dm.dropped_pairs(sc["p"], x, x, sc["real"], same=True) == 0
    i, j = spm.pm.pairs_within(x[:, :3], x[:, :3], sc["h"], real=sc["real"])
    off = np.abs(dm.cells(sc["p"], x, sc["real"])[j] - dm.cells(sc["p"], x, sc["real"])[i]).max(axis=1)
    assert (off == 1).any()
    assert dm.dropped_pairs(sc["p"], x, x, sc["real"], reach=0) == int((off > 0).sum())  # with a reach of 0 every pair across a face counts
    # the device's conversion: saturating, 0 for a NaN
    q = np.array([[1e30, -1e30, np.nan], [np.inf, -np.inf, 0.0]], sc["real"])
    c = dm.cells(sc["p"], q, sc["real"])
    assert c[0].tolist() == [2 ** 31 - 1, -2 ** 31, 0] and c[1, :2].tolist() == [2 ** 31 - 1, -2 ** 31]


@pytest.mark.parametrize("seed", SEEDS)
def test_no_pair_beyond_the_walk(seed):
    """particle-particle, particle-wall and query-particle pairs within h all lie within one cell of each other, and within 2 h within
    two (the anisotropic pass): the brute-force models see the device's candidates"""
    sc = scene(seed)
    assert fp.reader_dropped(sc, finite(sc), same=True) == 0
    q, attempt = fp.reader_queries_checked(sc)
    assert attempt == 0 and len(q) % 64 != 0 and fp.reader_dropped(sc, q[np.isfinite(q[:, :3]).all(axis=1)]) == 0
    lo = np.asarray(sc["p"]["worldOrigin"][0], np.float64)
    hi = lo + np.array(sc["gs"]) * np.asarray(sc["p"]["cellSize"][0], np.float64)
    w = q[40:80, :3].astype(np.float64)
    for t in range(40):  # beyond the box on the axis and side the row is drawn for
        a = t % 3
        assert w[t, a] >= hi[a] if (t // 3) % 2 else w[t, a] < lo[a], (t, w[t], lo, hi)
    sa = fp.make_reader_scene(seed, min_axis=8, max_particles=fp.ANISO_MAX_PARTICLES)
    r2h = float(sa["real"](2) * sa["real"](sa["p"]["interactionRadius"][0]))
    assert fp.reader_dropped(sa, sa["pos"], reach=2, radius=r2h, squared=True, same=True, walls=False) == 0


def test_the_query_sets_see_the_fluid():
    seen = 0
    for sd in (9400, 9404, 9411, 9417):
        sc = scene(sd)
        q, _ = fp.reader_queries_checked(sc)
        want = spm.sample(sc["p"], sc["pos"], sc["vel"], q, sc["kset"], sc["bi"] if sc["bi"] is None else np.concatenate((sc["bi"][:, :3], sc["vbi"][:, None]), axis=1))
        assert (want["count"][:40] >= 1).all() and not want["k"][80:84].any() and (want["count"] == 0).sum() > 10
        assert (want["k"][84:144] > want["count"][84:144]).sum() >= 50  # (queries that do see the wall)
        seen += int((want["count"] > 64).sum())
    assert seen > 20  # (sums longer than one 64-candidate load)


# ---- 3. the models' runs are not vacuous ----------------------------------------------------------------------------------------------------
def model_density(seed):
    if seed not in _dens:
        sc = scene(seed)
        origin, sp, dims = fp.reader_lattice(sc)
        assert np.prod(dims) <= fp.READER_MAX_NODES and min(dims) >= 2
        nodes = spm.lattice_points(origin, sp, dims, sc["real"])
        _dens[seed] = (origin, sp, dims, spm.sample(sc["p"], sc["pos"], sc["vel"], nodes, sc["kset"])["dens"].astype(sc["real"]))
    return _dens[seed]


def test_every_tetrahedron_case_occurs():
    total = np.zeros((6, 16), np.int64)
    complete = 0
    for sd in SEEDS:
        sc = scene(sd)
        origin, sp, dims, dens = model_density(sd)
        r = sfm.extract(dens, origin, sp, dims, 0.5 * float(sc["p"]["restDensity"][0]), sc["real"], tet_cases=True)
        h = r["tet_cases"]
        assert h.shape == (6, 16) and (h.sum(axis=1) == np.prod(np.array(dims) - 1)).all()
        sfm.mesh_checks(r["vertices"], r["triangles"], True)  # (the model's own surface is closed: the field is 0 on the border)
        complete += bool((h[:, 1:15] > 0).all())
        total += h
    print("tet cases: rarest (tetrahedron, case) pair %d times, %d scenes with all 84" % (total[:, 1:15].min(), complete))
    assert (total[:, 1:15] > 0).all() and total[:, 1:15].min() >= 20 and complete >= 3


def test_the_wall_term_changes_some_meshed_lattice():
    """SURFACE_WALLS is set on the even seeds (reader_surface_walls); on 9416 and 9422 the model's density with the wall term differs
    from the one without at hundreds of lattice nodes and flips the inside mask the mesh is cut from — a mesher that ignored the flag
    would not give the model's mesh there"""
    flagged = [sd for sd in SEEDS if fp.reader_surface_walls(sd)]
    assert len(flagged) == len(SEEDS) // 2
    flips = {}
    for sd in flagged:
        sc = scene(sd)
        if sc["bi"] is None:
            continue
        origin, sp, dims, plain = model_density(sd)
        sees = fp.reader_wall_nodes(sc, origin, sp, dims)
        if not sees.any():
            continue
        nodes = spm.lattice_points(origin, sp, dims, sc["real"])
        with_walls = spm.sample(sc["p"], sc["pos"], sc["vel"], nodes, sc["kset"], walls_of(sc))["dens"].astype(sc["real"])
        assert np.array_equal(with_walls[~sees], plain[~sees])
        iso = sc["real"](0.5 * float(sc["p"]["restDensity"][0]))
        flips[sd] = (int(sees.sum()), int(((with_walls >= iso) != (plain >= iso)).sum()))
    print("nodes that see a wall, inside-mask flips:", flips)
    assert sum(1 for n, f in flips.values() if n >= 100 and f >= 100) >= 2, flips


def test_tet_cases_of_a_hand_lattice():
    dens = np.zeros(8, np.float32)
    dens[0] = 1.0  # corner 000 inside: local corner 0 of all six tetrahedra
    h = sfm.extract(dens, (0, 0, 0), 1.0, (2, 2, 2), 0.5, np.float32, tet_cases=True)["tet_cases"]
    assert h[:, 1].tolist() == [1] * 6 and h.sum() == 6
    dens[:] = 0
    dens[1] = 1.0  # corner +x: local corner 1 of the tetrahedra xyz and xzy, outside all others
    h = sfm.extract(dens, (0, 0, 0), 1.0, (2, 2, 2), 0.5, np.float32, tet_cases=True)["tet_cases"]
    assert h[:2, 2].tolist() == [1, 1] and h[2:, 0].tolist() == [1] * 4
    assert "tet_cases" not in sfm.extract(dens, (0, 0, 0), 1.0, (2, 2, 2), 0.5, np.float32)


def test_the_diffuse_runs_show_everything():
    born, died, capped, overflowed, nonfinite_births = np.zeros(3, np.int64), 0, 0, 0, 0
    for sd in SEEDS:
        sc = scene(sd)
        cfg, cap, states, res = diffuse_run(sd)
        assert (cap is None or sd % 2 == 1) and len(res) == fp.READER_DIFFUSE_STEPS  # (a bounded capacity on odd seeds only)
        per_kind = np.zeros(3, np.int64)
        before = 0
        for r in res:
            F = r["F"]
            per_kind += np.bincount(np.repeat(F["parent_kind"], F["births"].astype(np.int64)), minlength=3)[:3]
            died += r["survivors"] < before
            before = r["alive"]
            capped += bool((r["births"] == cfg["max_per_particle"]).any())
            bad = ~np.isfinite(F["spos"]).all(axis=1)
            nonfinite_births += int(r["births"][bad].sum())
            assert bad.sum() == sc["nonfinite"]
        born = np.maximum(born, per_kind)
        overflowed += sum(r["dropped"] for r in res) > 0
    print("diffuse runs: most births of a kind on one seed %s, steps with deaths %d, with the cap %d, seeds that overflow %d" % (born, died, capped, overflowed))
    assert born.min() >= 50 and died > 0 and capped > 0 and overflowed >= 3, (born, died, capped, overflowed)
    assert nonfinite_births == 0  # a fluid particle with a non-finite coordinate has no neighbour, so no potential and no birth


def test_a_non_finite_particle_keeps_its_record():
    sc = scene(9423)
    assert sc["nonfinite"] > 0
    rec = record_for(np.where(np.isfinite(sc["pos"]), sc["pos"], 0), sc["real"])
    rec[-1, 0] = -0.0
    dt = 0.5 / tm.stability(sc["p"], sc["pos"], KAPPA, 1.0, sc["kset"])
    out = tm.diffuse(sc["p"], sc["pos"], rec, KAPPA, dt, sc["kset"])
    k = sc["nonfinite"]
    assert out[-k:].tobytes() == rec[-k:].tobytes() and np.count_nonzero(out[:-k, 0] != rec[:-k, 0]) > (sc["n"] - k) // 2
    assert out[:, 3].tobytes() == rec[:, 3].tobytes()


# ---- 4. the comparison notices: a model mutated in one place fails it on some seed --------------------------------------------------------
MUTATION_SEEDS = (9401, 9410, 9416, 9422)   # anisotropic cells, dense cells (ties), walls next to the fluid (9416, 9422), both kernel sets


def walls_of(sc):
    return None if sc["bi"] is None else np.concatenate((sc["bi"][:, :3], sc["vbi"][:, None]), axis=1).astype(sc["real"])


def as_device(want, real):
    """a model result in the arrays the device returns"""
    g4 = np.zeros((len(want["dens"]), 4), real)
    g4[:, :3] = want["grad"]
    return {spm.DENSITY: want["dens"].astype(real), spm.GRADIENT: g4, spm.VELOCITY: want["vel"].astype(real), spm.COUNT: want["count"].astype(np.uint32)}


def diffuse_bytes(sc):
    cfg = fp.reader_diffuse_config(sc)
    r = dm.step(sc["p"], cfg, sc["pos"], sc["vel"], np.zeros((0, 4), sc["real"]), np.zeros((0, 4), sc["real"]), 0, 0.0, sc["kset"])
    return b"".join(r[k].tobytes() for k in ("normals", "potentials", "births", "pos", "vel", "kind"))


def track_bytes(sc, walls):
    rec = record_for(np.where(np.isfinite(sc["pos"]), sc["pos"], 0), sc["real"])
    return tm.diffuse(sc["p"], sc["pos"], rec, KAPPA, 1e-4, sc["kset"], walls).tobytes()


def test_mutated_models_fail(monkeypatch):
    clean = {sd: (diffuse_bytes(scene(sd)), track_bytes(scene(sd), walls_of(scene(sd)))) for sd in MUTATION_SEEDS}
    for sd in MUTATION_SEEDS:  # (the unmutated model passes its own comparison)
        sc = scene(sd)
        q, _ = fp.reader_queries_checked(sc)
        want = spm.sample(sc["p"], sc["pos"], sc["vel"], q, sc["kset"], walls_of(sc))
        spm.compare(as_device(want, sc["real"]), want, "clean %d" % sd)

    # the wall term left out: the sampler's comparison and the attribute diffusion's bytes
    caught = 0
    for sd in MUTATION_SEEDS:
        sc = scene(sd)
        if sc["bi"] is None:
            continue
        q, _ = fp.reader_queries_checked(sc)
        dev = as_device(spm.sample(sc["p"], sc["pos"], sc["vel"], q, sc["kset"], walls_of(sc)), sc["real"])
        try:
            spm.compare(dev, spm.sample(sc["p"], sc["pos"], sc["vel"], q, sc["kset"], None), "no walls %d" % sd)
        except AssertionError:
            caught += 1
    assert caught >= 2, "the wall term left out goes unnoticed by the sampler's comparison"
    for sd in (9416, 9422):  # the two scenes whose fluid sees the wall: the attribute diffusion's density carries the wall term
        assert track_bytes(scene(sd), None) != clean[sd][1], "the wall term left out goes unnoticed by the attribute diffusion (%d)" % sd

    def differs():
        return [sd for sd in MUTATION_SEEDS if diffuse_bytes(scene(sd)) != clean[sd][0]], [sd for sd in MUTATION_SEEDS if track_bytes(scene(sd), walls_of(scene(sd))) != clean[sd][1]]

    # one of the 27 cells left out
    real_walk = dm.walk_pairs

    def walk_without_a_cell(params, x, y, real, same=False):
        i, j, d = real_walk(params, x, y, real, same)
        off = dm.cells(params, np.asarray(y)[:, :3].astype(real), real)[j] - dm.cells(params, np.asarray(x)[:, :3].astype(real), real)[i]
        keep = ~((off[:, 0] == 1) & (off[:, 1] == 0) & (off[:, 2] == -1))
        return i[keep], j[keep], d[keep]
    monkeypatch.setattr(dm, "walk_pairs", walk_without_a_cell)
    a, b = differs()
    assert a and b, "a cell left out goes unnoticed"
    monkeypatch.setattr(dm, "walk_pairs", real_walk)

    # cellSize axes swapped in cells
    real_grid = dm._grid

    def grid_swapped(params, real):
        wo, cs, gs = real_grid(params, real)
        return wo, cs[[1, 0, 2]], gs
    monkeypatch.setattr(dm, "_grid", grid_swapped)
    a, b = differs()
    assert a and b and all(np.ptp(scene(sd)["cs"][:2]) > 0 for sd in a + b), "swapped cell sizes go unnoticed"
    monkeypatch.setattr(dm, "_grid", real_grid)

    # the tie order of sorted_order reversed
    def order_reversed(params, pos, real):
        _, _, gs = dm._grid(params, real)
        c = dm.cells(params, pos, real) & (gs - 1)
        h = (c[:, 2] * gs[1] + c[:, 1]) * gs[0] + c[:, 0]
        return np.lexsort((-np.arange(len(h)), h))
    monkeypatch.setattr(dm, "sorted_order", order_reversed)
    a, b = differs()
    assert a and b, "a reversed tie order goes unnoticed"
    monkeypatch.undo()
    assert differs() == ([], [])
