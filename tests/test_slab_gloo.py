"""Slab decomposition over torch.distributed: world_size 2 and 3 with the gloo backend.

CPU (not gpu): the exchange protocol of nereus_amd.slab.SlabDriver with a checker engine (numpy partitioning +
CPU oracle physics).  GPU (-m gpu): the same protocol with the product engine (HipSlabEngine: device-side
partition/pack/unpack + HIP step), two ranks sharing the one GPU of the test box, messages staged through host
memory because gloo cannot carry device tensors (on a multi-GPU node the backend is nccl = RCCL over xGMI).
Both are compared with the single-domain oracle on the union scene, particle by particle through an id carried
in vel.w (tolerance: the slab path orders in-cell sums differently).
The checker engine's partition is tests/slab_model.py, the numpy statement that tests/test_slab_partition_gpu.py compares the device's
streams with bit for bit: the protocol tests and the device tests share one statement of nrs_slab_pack / nrs_slab_unpack.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICE = (9, 8, 7)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _base_params(double, kset):
    """constructor defaults in the build's precision (the kernel set changes none of them), as tools/fuzz_slab.py takes them"""
    from nereus_amd.params import default_params

    return default_params(0, double=double)


def _worker(rank, world, port, steps, use_hip, outdir, skew=0, rebalance_every=0, lattice=None, double=False, kset=1):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from nereus_amd import scene, slab

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lattice = lattice or LATTICE
    real = np.float64 if double else np.float32
    assert use_hip or real is np.float32   # (the checker engine is fp32 Muller)
    p, cuts, pos, vel, bi, vbi, info = slab.rank_scene(lattice, rank, world, _base_params(double, kset), real=real)
    # particle id rides in vel.w (preserved by reorder/integrate/exchange): global lattice id
    nx, ny, nz = lattice
    d = float(real(p["interactionRadius"][0])) - 0.005
    ix = np.rint(pos[:, 0] / d - 1).astype(np.int64)
    iy = np.rint(pos[:, 1] / d - 1).astype(np.int64)
    iz = np.rint(pos[:, 2] / d - 1).astype(np.int64)
    vel[:, 3] = ((ix * ny + iy) * nz + iz).astype(real)
    vel[:, 0] = np.where((iy + iz) % 2 == 0, 2.5, -2.5).astype(real)  # make particles cross the cuts
    if skew:  # deliberately unbalanced cuts (every interior cut moved by `skew` cells) to exercise the re-cut
        cuts = [cuts[0]] + [c + skew for c in cuts[1:-1]] + [cuts[-1]]
        ox, cs = float(p["worldOrigin"][0][0]), float(p["cellSize"][0][0])
        full = scene.fluid_block(nx * world, ny, nz, float(p["interactionRadius"][0]))
        cx = slab.cell_of(full[:, 0], ox, cs)
        mine = (cx >= cuts[rank]) & (cx < cuts[rank + 1])
        pos = full[mine]
        vel = np.zeros_like(pos)
        ix = np.rint(pos[:, 0] / d - 1).astype(np.int64)
        iy = np.rint(pos[:, 1] / d - 1).astype(np.int64)
        iz = np.rint(pos[:, 2] / d - 1).astype(np.int64)
        vel[:, 3] = ((ix * ny + iy) * nz + iz).astype(np.float32)
        vel[:, 0] = np.where((iy + iz) % 2 == 0, 2.5, -2.5).astype(np.float32)
        full_scene = scene.dam_break((nx * world, ny, nz), h=float(p["interactionRadius"][0]), kpoly=float(p["kpoly"][0]))
        bi, vbi = full_scene["bi"], full_scene["vbi"]  # every rank sees the whole (small) tank: cuts will move
    msg_cap, ctx_cap = 4096, 8192
    if lattice != LATTICE:
        msg_cap, ctx_cap = slab.capacities(lattice, float(p["interactionRadius"][0]), len(pos))
    if use_hip:
        eng = slab.HipSlabEngine(p, ctx_cap, msg_cap, cuts[rank], cuts[rank + 1], 0, double=double, kernel_set=kset)
    else:
        from tests.slab_check_engine import OracleSlabEngine

        eng = OracleSlabEngine(p, msg_cap, cuts[rank], cuts[rank + 1])
    eng.load(pos, vel, bi, vbi)
    drv = slab.SlabDriver(eng, rank, world, stage_through_host=use_hip)
    moved = 0
    owned_hist = [len(pos)]
    for it in range(steps):
        if rebalance_every and it % rebalance_every == 0:
            drv.rebalance(int(p["gridSize"][0][0]), move_budget=msg_cap // 2)
        drv.exchange()
        moved += drv.last_counts[1] + drv.last_counts[3]
        owned_hist.append(eng.n_owned)
        if os.environ.get("NEREUS_TEST_TRACE"):
            print("TRACE rank %d it %d owned %d local %d counts %s cuts %s resort %s" % (rank, it, eng.n_owned, eng.n_local, list(drv.last_counts),
                                                                          (eng.cell_lo, eng.cell_hi), eng.solver.resort_stats() if use_hip else None), flush=True)
        eng.step(1)
    drv.finish()
    moved += drv.last_counts[1] + drv.last_counts[3]
    op, ov = eng.owned_state()
    resort = np.array(eng.solver.resort_stats() if use_hip else (0, 0))
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), pos=op, vel=ov, moved=moved, cuts=np.array(cuts[1:-1]),
             params=p.view(np.uint8), owned=np.array(owned_hist), resort=resort)
    dist.barrier()
    dist.destroy_process_group()


def _run(world, steps, use_hip, tmp_path, skew=0, rebalance_every=0, lattice=None, double=False, kset=1, tol=1e-5, cut_off_margin=0.0):
    """cut_off_margin > 0: before anything is compared, no pair of the oracle's run comes closer than that to the cut-off radius
    (tests/slab_scenes.py cut_off_margin: the truncated Monaghan kernels jump there)"""
    from nereus_amd import scene
    from nereus_amd.params import params_dtype
    from tests.common import rel_err
    from tests.oracle_lib import SESPH, Oracle

    lattice = lattice or LATTICE
    real = np.float64 if double else np.float32
    mp.spawn(_worker, args=(world, _free_port(), steps, use_hip, str(tmp_path), skew, rebalance_every, lattice, double, kset),
             nprocs=world, join=True)
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    pos = np.concatenate([q["pos"] for q in parts])
    vel = np.concatenate([q["vel"] for q in parts])
    nx, ny, nz = lattice
    n = nx * world * ny * nz
    assert len(pos) == n, "particles lost or duplicated by the exchange"
    ids = vel[:, 3].astype(np.int64)
    assert np.array_equal(np.sort(ids), np.arange(n))
    # single-domain oracle on the union scene with the same global grid
    p = parts[0]["params"].view(params_dtype(double)).copy()
    h = float(p["interactionRadius"][0])
    full = scene.dam_break((nx * world, ny, nz), h=h, kpoly=float(p["kpoly"][0]), real=real)
    fvel = full["vel"].copy()
    fvel[:, 3] = np.arange(n, dtype=real)
    gid = np.arange(n)
    fvel[:, 0] = np.where(((gid // nz) % ny + gid % nz) % 2 == 0, 2.5, -2.5).astype(real)
    o = Oracle(p, double, kset, SESPH, threads=min(16, os.cpu_count() or 1), tait="double7" if double else "powf")
    o.set_particles(full["pos"], fvel)
    o.set_boundaries(full["bi"], full["vbi"], update_grid=True)
    np.testing.assert_array_equal(o.params.view(np.uint8), p.view(np.uint8))  # same GLOBAL grid on every rank
    if cut_off_margin:
        from tests.slab_scenes import cut_off_margin as margin_of

        states = [(full["pos"], fvel)]
        for _ in range(steps):
            o.step(1)
            states.append((o.get("pos").copy(), None))
        assert margin_of(states, h) >= cut_off_margin, margin_of(states, h)
    else:
        o.step(steps)
    rp, rv = o.get("pos"), o.get("vel")
    order_ref = np.argsort(rv[:, 3].astype(np.int64))
    order_got = np.argsort(ids)
    e_p, e_v = rel_err(pos[order_got][:, :3], rp[order_ref][:, :3]), rel_err(vel[order_got][:, :3], rv[order_ref][:, :3])
    print("slab gloo %s kset %d, %d ranks, %d steps against the oracle: pos %.3g vel %.3g (bar %.0e)"
          % ("f64" if double else "f32", kset, world, steps, e_p, e_v, tol))
    assert e_p <= tol
    assert e_v <= tol
    _run.owned = [q["owned"] for q in parts]
    _run.resort = [tuple(int(v) for v in q["resort"]) for q in parts]
    return sum(int(q["moved"]) for q in parts)


@pytest.mark.parametrize("world", [2, 3])
def test_slab_protocol_gloo_cpu(tmp_path, world):
    assert _run(world, 12, False, tmp_path) > 0  # some particles changed owner


@pytest.mark.gpu
def test_slab_hip_engine_two_ranks_one_gpu(tmp_path, hip_lib):
    assert _run(2, 25, True, tmp_path) > 0


@pytest.mark.gpu
def test_slab_hip_engine_fp64_monaghan(tmp_path, hip_lib):
    """the product driver and engine in the fp64 Monaghan build (HipSlabEngine(double=True, kernel_set=MONAGHAN)): 12 steps against
    the fp64 Monaghan oracle at TOL_STEPS_F64, no pair within 1e-11 m of the cut-off radius during the oracle's run"""
    from nereus_amd import capi
    from tests.test_parity_gpu import TOL_STEPS_F64

    assert _run(2, 12, True, tmp_path, double=True, kset=capi.MONAGHAN, tol=TOL_STEPS_F64, cut_off_margin=1e-11) > 0


@pytest.mark.gpu
def test_slab_hip_engine_coherent_resort(tmp_path, hip_lib):
    """Slabs big enough for the coherent re-sort (>= 32768 local particles): after the partition the owned particles
    that stayed in their cell are merged with the sorted rest (cell changers, arrivals, halo copies) instead of a
    full sort; same bar against the single-domain oracle, and the path must really have been taken."""
    steps = 10
    assert _run(2, steps, True, tmp_path, lattice=(48, 28, 26)) > 0
    for used, fallbacks in _run.resort:
        # a fall-back (more than 1/8 of the local particles are cell changers + arrivals + halo copies) is legitimate in
        # a slab this narrow, but most steps must have merged
        assert used >= steps - 1 and fallbacks <= used // 3


@pytest.mark.gpu
def test_slab_c4_per_rank_size(tmp_path, hip_lib):
    """BASELINE config C4 at its per-rank size: the 16 M-particle run gives every GPU a 32 x 250 x 250 = 2 M-particle slab
    (256 x 250 x 250 over 8 ranks).  Two such ranks share the one GPU of the test box (gloo + host staging instead of RCCL);
    10 steps with particles crossing the cut; particle ids conserved, state finite, every step after the first on the merge
    path of the coherent re-sort, and positions / velocities within 1e-5 of the single-domain ORACLE on the 64 x 250 x 250
    union, particle by particle."""
    steps = 10
    moved = _run(2, steps, True, tmp_path, lattice=(32, 250, 250))
    assert moved > 1000
    for used, fallbacks in _run.resort:
        assert used >= steps - 1 and fallbacks == 0
    owned = np.stack(_run.owned)
    assert owned.sum(axis=0).tolist() == [2 * 32 * 250 * 250] * (steps + 1)


@pytest.mark.gpu
def test_slab_rebalance_with_fused_classification(tmp_path, hip_lib):
    """Slabs big enough for the in-place partition, whose classification rides in the force kernel: a re-cut between the
    step and the partition invalidates that classification (it was made for the old cuts); same bar against the
    single-domain oracle, counts converge."""
    moved = _run(2, 9, True, tmp_path, skew=-3, rebalance_every=3, lattice=(48, 28, 26))
    owned = np.stack(_run.owned)
    assert abs(int(owned[0, -1]) - int(owned[1, -1])) < abs(int(owned[0, 0]) - int(owned[1, 0])) and moved > 0
    for used, fallbacks in _run.resort:
        assert used >= 4


def test_message_capacity_rule_covers_the_halo():
    """bench.py sizes the fixed message buffers from the lattice; check the rule against real partition counts."""
    sys.path.insert(0, ROOT)
    from nereus_amd import slab
    from nereus_amd.params import default_params
    from tests.slab_check_engine import OracleSlabEngine

    lattice, world = (24, 20, 18), 3
    for rank in range(world):
        p, cuts, pos, vel, bi, vbi, info = slab.rank_scene(lattice, rank, world, default_params(0))
        msg_cap, cap = slab.capacities(lattice, float(p["interactionRadius"][0]), len(pos))
        eng = OracleSlabEngine(p, msg_cap, cuts[rank], cuts[rank + 1])
        eng.load(pos, vel, bi, vbi)
        left = eng.make_buffer() if rank > 0 else None
        right = eng.make_buffer() if rank < world - 1 else None
        stay, ml, hl, mr, hr, gh = eng.pack(left, right)
        assert stay == len(pos) and ml == mr == gh == 0
        assert max(hl, hr) * 1.3 <= msg_cap and stay + 2 * max(hl, hr) <= cap
        if rank > 0:
            assert hl > 0
        assert abs(len(pos) - np.prod(lattice)) <= 2 * lattice[1] * lattice[2]  # count-balanced to within two planes


def test_new_cuts_rule():
    from nereus_amd.slab import NO_CUT_HI, NO_CUT_LO, new_cuts

    hist = np.zeros(64, np.int64)
    hist[10:30] = 100                                     # 2000 particles in columns 10..29
    old = [NO_CUT_LO, 14, NO_CUT_HI]
    assert new_cuts(hist, old, 2, 10 ** 9) == [NO_CUT_LO, 20, NO_CUT_HI]          # unconstrained: the median column
    assert new_cuts(hist, old, 2, 250) == [NO_CUT_LO, 16, NO_CUT_HI]              # budget: two columns of 100 fit, three do not
    old3 = [NO_CUT_LO, 12, 16, NO_CUT_HI]
    got = new_cuts(hist, old3, 2, 10 ** 9)
    assert got[1] == 12 and got[2] == 24                  # cut 1 may not pass old cut 2 minus two halos; cut 2 reaches the 2/3 column
    assert all(b - a >= 4 for a, b in zip(got[1:-2], got[2:-1]))


def test_slab_rebalance_gloo_cpu(tmp_path):
    """Start with cuts 3 cells off balance; re-cut every 2 steps under the message budget: the owned counts converge and
    the result still equals the single-domain oracle."""
    moved = _run(2, 10, False, tmp_path, skew=-3, rebalance_every=2)
    owned = np.stack(_run.owned)          # (rank, step)
    imbalance0 = abs(int(owned[0, 0]) - int(owned[1, 0]))
    imbalance1 = abs(int(owned[0, -1]) - int(owned[1, -1]))
    assert imbalance0 > 0 and imbalance1 < imbalance0 and moved > 0


@pytest.mark.gpu
def test_slab_rebalance_hip_engine(tmp_path, hip_lib):
    moved = _run(2, 12, True, tmp_path, skew=-3, rebalance_every=2)
    owned = np.stack(_run.owned)
    assert abs(int(owned[0, -1]) - int(owned[1, -1])) < abs(int(owned[0, 0]) - int(owned[1, 0])) and moved > 0


# ---------------------------------------------------------------- IISPH over slabs
IISPH_LATTICE = (22, 8, 8)


def _iisph_scene(double=False, kset=1):
    """A compressed block (so that the pressure solve has work) under the IISPH constructor defaults: global 128^3 grid."""
    from nereus_amd import scene
    from nereus_amd.params import default_params

    real = np.float64 if double else np.float32
    p = default_params(1, double=double)   # (the kernel set changes none of the constructor defaults)
    h = float(p["interactionRadius"][0])
    pos = scene.fluid_block(*IISPH_LATTICE, h, real=real, jitter=0.02, spacing=0.72 * h)
    vel = np.zeros_like(pos)
    vel[:, 0] = np.where((np.arange(len(pos)) // IISPH_LATTICE[2]) % 2 == 0, 1.5, -1.5).astype(real)  # cross the cut
    return p, pos, vel


def _iisph_worker(rank, world, port, steps, use_hip, outdir, by_slot, force_iters=0, halo=None, double=False, kset=1):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from nereus_amd import capi, slab

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    p, pos, vel = _iisph_scene(double, kset)
    ox, cs = float(p["worldOrigin"][0][0]), float(p["cellSize"][0][0])
    cx = slab.cell_of(pos[:, 0], ox, cs, real=pos.dtype.type)
    cut = int(np.median(cx)) + 1
    cuts = [slab.NO_CUT_LO, cut, slab.NO_CUT_HI]
    mine = (cx >= cuts[rank]) & (cx < cuts[rank + 1])
    halo = halo or slab.IISPH_HALO_CELLS
    if use_hip:
        eng = slab.HipSlabEngine(p, 4 * len(pos), 2 * len(pos), cuts[rank], cuts[rank + 1], 0, halo=halo, iisph=True,
                                 flags=capi.FLAG_IISPH_SELF_BY_SLOT if by_slot else 0, double=double, kernel_set=kset)
    else:
        from tests.slab_check_engine import OracleSlabEngine

        assert not double and kset == 1   # (the checker engine is fp32 Muller)

        eng = OracleSlabEngine(p, 2 * len(pos), cuts[rank], cuts[rank + 1], halo=halo, iisph=True, self_by_slot=by_slot)
    eng.load(pos[mine], vel[mine], None, None)
    drv = slab.SlabDriver(eng, rank, world, stage_through_host=use_hip)
    iters, moved = [], 0
    for _ in range(steps):
        drv.exchange()
        moved += drv.last_counts[1] + drv.last_counts[3]
        iters.append(drv.iisph_step(min_iters=force_iters or 2))
    drv.finish()
    op, ov = eng.owned_state()
    np.savez(os.path.join(outdir, "irank%d.npz" % rank), pos=op, vel=ov, iters=np.array(iters), moved=moved,
             truncated=drv.truncated_steps)
    dist.barrier()
    dist.destroy_process_group()


def _iisph_single(p, pos0, vel0, steps, by_slot, force_iters=0, double=False, kset=1):
    from tests.oracle_lib import IISPH, Oracle

    o = Oracle(p, double, kset, solver=IISPH, self_by_slot=by_slot, tait="double7" if double else "powf")
    o.set_particles(pos0, vel0)
    o.set_boundaries(None, None)
    iters = []
    for _ in range(steps):
        o.step(1, max_iters=-force_iters)   # (negative: exactly that many iterations, nereus_oracle.cpp iisphStep)
        iters.append(o.last_iters)
    return o.get("pos"), o.get("vel"), iters


def _match(ref_pos, pos):
    """both w components are overwritten by iisph_integrate, so no id survives a step: pair the particles by position
    (lattice spacing 0.039 m); returns (distances, index into ref)"""
    from scipy.spatial import cKDTree

    return cKDTree(ref_pos[:, :3]).query(pos[:, :3])


def _run_iisph(steps, use_hip, tmp_path, by_slot, force_iters=0, halo=None, single_iters=None, double=False, kset=1):
    mp.spawn(_iisph_worker, args=(2, _free_port(), steps, use_hip, str(tmp_path), by_slot, force_iters, halo, double, kset), nprocs=2,
             join=True)
    parts = [np.load(os.path.join(str(tmp_path), "irank%d.npz" % r)) for r in range(2)]
    pos = np.concatenate([q["pos"] for q in parts])
    vel = np.concatenate([q["vel"] for q in parts])
    p, pos0, vel0 = _iisph_scene(double, kset)
    assert len(pos) == len(pos0), "particles lost or duplicated by the exchange"
    assert sum(int(q["moved"]) for q in parts) > 0
    rp, rv, ref_iters = _iisph_single(p, pos0, vel0, steps, by_slot, force_iters if single_iters is None else single_iters, double, kset)
    assert list(parts[0]["iters"]) == ref_iters == list(parts[1]["iters"])   # the global exit test, same count on every rank
    _run_iisph.truncated = [int(q["truncated"]) for q in parts]
    d, idx = _match(rp, pos)
    return pos, vel, rp, rv, d, idx


def _check_order_independent(steps, use_hip, tmp_path, force_iters=0, halo=None, single_iters=None, double=False, kset=1,
                             tol=(1e-5, 1e-4)):
    """NRS_FLAG_IISPH_SELF_BY_SLOT (SURVEY Q5 off): the result no longer depends on the order of the arrays, so two slabs must
    reproduce the single-domain oracle particle for particle — this is the test of the halo width, of the pressure carried in
    vel.w and of the all-reduced exit test."""
    from tests.common import rel_err

    pos, vel, rp, rv, d, idx = _run_iisph(steps, use_hip, tmp_path, True, force_iters, halo, single_iters, double, kset)
    assert len(np.unique(idx)) == len(pos) and d.max() < 1e-5
    e_p, e_v = rel_err(pos[:, :3], rp[idx, :3]), rel_err(vel[:, :3], rv[idx, :3])
    print("slab gloo iisph by slot %s kset %d, %d steps against the oracle: pos %.3g vel %.3g (bars %.0e / %.0e)"
          % ("f64" if double else "f32", kset, steps, e_p, e_v, tol[0], tol[1]))
    assert e_p <= tol[0]
    assert e_v <= tol[1]


def _check_reference_mode(steps, use_hip, tmp_path):
    """Default flags = the reference's Q5 self-exclusion by thread id: its result depends on the ORDER of the input arrays, and a
    slab's local order is not the single domain's.  The yardstick is the single-domain oracle run on a permutation of the same
    particles: the slab run must not be further from the single-domain run than that permuted run is."""
    pos, vel, rp, rv, d, idx = _run_iisph(steps, use_hip, tmp_path, False)
    p, pos0, vel0 = _iisph_scene()
    perm = np.random.default_rng(1).permutation(len(pos0))
    pp, _, _ = _iisph_single(p, pos0[perm], vel0[perm], steps, False)
    dy, _ = _match(rp, pp)
    print("IISPH, reference self-exclusion: slabs vs single domain max %.3e m (rms %.3e); permuted single domain max %.3e m (rms %.3e)"
          % (d.max(), np.sqrt((d * d).mean()), dy.max(), np.sqrt((dy * dy).mean())))
    assert dy.max() > 1e-3, "the yardstick itself: a permutation alone must move particles by millimetres"
    assert d.max() <= 1.5 * dy.max() and np.sqrt((d * d).mean()) <= 1.5 * np.sqrt((dy * dy).mean())


def test_iisph_slabs_gloo_cpu(tmp_path):
    """IISPH over two slabs with the checker engine: 8-cell halo, pressure carried in vel.w, solver loop exit decided on the
    all-reduced density error — against the single-domain oracle."""
    _check_order_independent(4, False, tmp_path)


def test_iisph_slabs_reference_mode_gloo_cpu(tmp_path):
    _check_reference_mode(4, False, tmp_path)


@pytest.mark.gpu
def test_iisph_slabs_hip_engine(tmp_path, hip_lib):
    _check_order_independent(6, True, tmp_path)


@pytest.mark.gpu
def test_iisph_slabs_hip_engine_fp64_muller(tmp_path, hip_lib):
    """the fp64 Muller build through the product driver: SlabDriver.iisph_step forms its mean density in float64 (engine.double);
    self-exclusion by slot, against the fp64 oracle at TOL_STEPS_F64"""
    from nereus_amd import capi
    from tests.test_parity_gpu import TOL_STEPS_F64

    _check_order_independent(6, True, tmp_path, double=True, kset=capi.MULLER, tol=(TOL_STEPS_F64, TOL_STEPS_F64))


@pytest.mark.gpu
def test_iisph_slabs_reference_mode_hip_engine(tmp_path, hip_lib):
    _check_reference_mode(6, True, tmp_path)


# The reference's exit test leaves its loop after two iterations on every scene tried (its relaxed Jacobi overshoots: the mean
# corrected density goes far below 1000 after the second sweep), so longer solves are driven through SlabDriver.iisph_step's
# min_iters — the halo budget 2 * iterations + 4 is what these tests are about.
def test_iisph_slabs_four_iterations_gloo_cpu(tmp_path):
    """Four solver iterations per step over a 12-cell halo (slab.iisph_halo_cells(4)) reproduce the single-domain oracle driven
    through the same four iterations, particle for particle."""
    from nereus_amd import slab

    assert slab.iisph_halo_cells(4) == 12 and slab.iisph_halo_cells(1) == 8
    _check_order_independent(3, False, tmp_path, force_iters=4, halo=12)
    assert _run_iisph.truncated == [0, 0]


@pytest.mark.gpu
def test_iisph_slabs_four_iterations_hip_engine(tmp_path, hip_lib):
    _check_order_independent(4, True, tmp_path, force_iters=4, halo=12)
    assert _run_iisph.truncated == [0, 0]


@pytest.mark.gpu
def test_iisph_slabs_iteration_cap_is_reported_not_fatal(tmp_path, hip_lib):
    """A step that wants more iterations than the halo supports (8 cells = 2 iterations, 4 asked for) is finished at the cap on
    every rank and counted — the run goes on, the contexts are not left mid-step — and equals the single domain capped alike."""
    _check_order_independent(4, True, tmp_path, force_iters=4, halo=8, single_iters=2)
    assert _run_iisph.truncated == [4, 4]


# ---------------------------------------------------------------- the exchange driven from C++ over RCCL
@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["sesph", "iisph"])
def test_slab_rccl_cpp_driver_one_rank(tmp_path, hip_lib, solver):
    """nereus_amd/host/tools/slab_rccl.cpp (RCCL send/recv + all-reduce on the context's stream, no interpreter in the loop), as far as a
    one-GPU box can run it: RCCL refuses two ranks on one device (tools/probe_rccl_same_gpu.py), so ONE rank — communicator
    bootstrap through the id file, the pack / (no neighbour) / unpack bracket every step, for IISPH the all-reduced exit test — against
    a single-domain context of the same scene.  With more ranks the same binary exchanges over xGMI; that path has never run."""
    import subprocess

    sys.path.insert(0, ROOT)
    from nereus_amd import capi, slab
    from nereus_amd.params import default_params
    from tests.common import rel_err

    exe = os.path.join(ROOT, "nereus_amd", "nereus_slab_rccl")
    assert os.path.exists(exe), "build it: make -C nereus_amd/host"
    iisph = solver == "iisph"
    if iisph:
        p, pos, vel = _iisph_scene()
        bi = vbi = None
        halo, steps = 8, 4
    else:
        p, cuts, pos, vel, bi, vbi, info = slab.rank_scene((24, 20, 18), 0, 1, default_params(0))
        halo, steps = 2, 12
    ids = np.arange(len(pos), dtype=np.float32)
    if not iisph:
        vel = vel.copy(); vel[:, 3] = ids
    scene_file, out_file = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    slab.write_rank_scene(scene_file, p, slab.NO_CUT_LO, slab.NO_CUT_HI, halo, 8192, 4 * len(pos), pos, vel, bi, vbi, iisph=iisph)
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", NEREUS_NCCL_ID_FILE=str(tmp_path / "nccl.id"),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([exe, scene_file, str(steps), out_file], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-1500:])
    gp, gv, trunc, iters = slab.read_rank_result(out_file)
    assert len(gp) == len(pos) and trunc == 0
    s = capi.Solver(p, len(pos), solver=capi.IISPH if iisph else capi.SESPH, flags=capi.FLAG_IISPH_SELF_BY_SLOT if iisph else 0)
    s.set_particles(pos, vel)
    s.set_boundaries(bi, vbi, update_grid=False)
    s.step(steps)
    rp, rv = s.download()
    if iisph:
        assert iters == s.last_iterations
        d, idx = _match(rp, gp)
        assert len(np.unique(idx)) == len(gp) and d.max() < 1e-5
        assert rel_err(gv[:, :3], rv[idx, :3]) <= 1e-4
    else:
        a, b = np.argsort(gv[:, 3], kind="stable"), np.argsort(rv[:, 3], kind="stable")
        assert np.array_equal(gv[a, 3], ids)
        assert rel_err(gp[a, :3], rp[b, :3]) <= 1e-5 and rel_err(gv[a, :3], rv[b, :3]) <= 1e-5


@pytest.mark.gpu
def test_slab_pack_defers_its_totals(hip_lib):
    """include/nereus_hip.h: nrs_slab_pack(counts = NULL) queues the partition and returns; the stream totals are read back by
    nrs_slab_unpack (together with the received headers) or by whichever call needs the particle count first — and a message-capacity
    overflow is then reported there, not lost."""
    import ctypes as C

    sys.path.insert(0, ROOT)
    from nereus_amd import capi, slab
    from nereus_amd.params import default_params
    from tests.common import rel_err

    p, cuts, pos, vel, bi, vbi, info = slab.rank_scene((20, 16, 14), 0, 1, default_params(0))
    n = len(pos)
    s = capi.Solver(p, 2 * n)
    s.set_particles(pos, vel)
    s.set_boundaries(bi, vbi, update_grid=False)
    s.slab_configure(slab.NO_CUT_LO, slab.NO_CUT_HI, 2)
    # (a) open slab, no neighbours: pack without counts, the next call that needs n settles it
    assert s.slab_pack(None, None, 4096, want_counts=False) is None
    assert s.n == n and s.slab_last_counts() == [n, 0, 0, 0, 0, 0]
    s.slab_unpack(None, None, 4096)
    s.step(2)
    r = capi.Solver(p, 2 * n)
    r.set_particles(pos, vel)
    r.set_boundaries(bi, vbi, update_grid=False)
    r.step(2)
    a, b = s.download(), r.download()
    assert rel_err(np.sort(a[0][:, 0]), np.sort(b[0][:, 0])) <= 1e-5
    # (b) a cut through the block and a message buffer far too small: the pack itself returns, the overflow surfaces at the next call
    shim = C.CDLL(os.path.join(ROOT, "nereus_amd", "libnereus_refshim.so"))
    shim.allocateArray.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    buf = C.c_void_p()
    cap = 64
    shim.allocateArray(C.byref(buf), s.message_bytes(cap))
    t = capi.Solver(p, 2 * n)
    t.set_particles(pos, vel)
    t.set_boundaries(bi, vbi, update_grid=False)
    cx = slab.cell_of(pos[:, 0], float(p["worldOrigin"][0][0]), float(p["cellSize"][0][0]))
    t.slab_configure(slab.NO_CUT_LO, int(np.median(cx)), 2)      # everything right of the median cell has to leave to the right
    assert t.slab_pack(None, buf, cap, want_counts=False) is None
    with pytest.raises(capi.NereusError, match="capacity"):
        t.slab_unpack(None, None, cap)
    shim.freeArray.argtypes = [C.c_void_p]
    t.close()
    shim.freeArray(buf)
