"""The ranks of a slab run as contexts of ONE process on one GPU, without torch and without a process group (a helper module of
tests/test_slab_builds_gpu.py, not a test): `world` capi.Solver contexts of one build (precision x kernel set), each configured with
its cuts and halo and holding the whole (small) tank as boundaries.  The neighbour exchange needs no copy: nrs_slab_unpack only reads
its inputs, so every rank unpacks straight from its neighbours' send buffers once all packs have finished.  Everything else
(nrs_slab_pack / _unpack, nrs_step, nrs_iisph_predict / _iterate / _finish) is the product code; the IISPH exit test forms its mean
density with nereus_amd.slab.mean_density, as SlabDriver.iisph_step and tools/fuzz_slab.py do."""
import numpy as np

from nereus_amd import capi, slab
from tests.test_slab_partition_gpu import Buffer

STAY, MIG_L, HALO_L, MIG_R, HALO_R, GHOST = range(6)   # order of the six counts of nrs_slab_pack (tests/slab_model.py STREAMS)


class SlabRanks:
    def __init__(self, params, cuts, halo, capacity, msg_capacity, double=False, kernel_set=capi.MULLER, solver=capi.SESPH,
                 reference_order=False, flags=0):
        """cuts: world + 1 cell-x indices, the outer two open (slab.NO_CUT_LO / NO_CUT_HI)"""
        self.params, self.cuts, self.halo = params, list(cuts), int(halo)
        self.world = len(cuts) - 1
        self.double, self.real = bool(double), (np.float64 if double else np.float32)
        self.iisph = solver == capi.IISPH
        self.max_iters = (self.halo - 4) // 2 if self.iisph else None
        self.msg_capacity = int(msg_capacity)
        self.ranks, self.send_l, self.send_r = [], [], []
        self.totals = np.zeros((self.world, 6), np.int64)   # the pack counts of every rank, summed over the exchanges
        self.truncated_steps = 0
        self.last_iterations = None
        for r in range(self.world):
            s = capi.Solver(params, capacity, solver=solver, double=double, kernel_set=kernel_set, reference_order=reference_order,
                            flags=flags)
            self.ranks.append(s)
            nbytes = s.message_bytes(self.msg_capacity)
            self.send_l.append(Buffer(nbytes) if r > 0 else None)
            self.send_r.append(Buffer(nbytes) if r < self.world - 1 else None)

    def cell_x(self, x):
        p = self.params
        return slab.cell_of(x, p["worldOrigin"][0][0], p["cellSize"][0][0], real=self.real)

    def load(self, pos, vel, bi=None, vbi=None, pres=None):
        """every rank gets the particles of its cells (in the order given) and the whole tank"""
        cx = self.cell_x(pos[:, 0])
        for r, s in enumerate(self.ranks):
            mine = (cx >= self.cuts[r]) & (cx < self.cuts[r + 1])
            s.set_particles(pos[mine], vel[mine], None if pres is None else pres[mine])
            s.set_boundaries(bi, vbi, update_grid=False)
            s.slab_configure(self.cuts[r], self.cuts[r + 1], self.halo)

    def set_cut(self, k, cell):
        """move the interior cut k (between rank k - 1 and rank k); both neighbours are told before the next exchange"""
        self.cuts[k] = int(cell)
        for r in (k - 1, k):
            self.ranks[r].slab_configure(self.cuts[r], self.cuts[r + 1], self.halo)

    @staticmethod
    def _ptr(b):
        return None if b is None else b.ptr

    def exchange(self):
        """pack on every rank (no wait), wait for every rank, unpack from the neighbours' send buffers; returns the counts per rank"""
        ptr, cap = self._ptr, self.msg_capacity
        for r, s in enumerate(self.ranks):
            assert s.slab_pack(ptr(self.send_l[r]), ptr(self.send_r[r]), cap, want_counts=False) is None
        for s in self.ranks:
            s.synchronize()
        for r, s in enumerate(self.ranks):
            s.slab_unpack(ptr(self.send_r[r - 1]) if r > 0 else None, ptr(self.send_l[r + 1]) if r < self.world - 1 else None, cap)
        counts = []
        for r, s in enumerate(self.ranks):
            s.synchronize()    # the next pack of a neighbour overwrites what this unpack has read
            counts.append(s.slab_last_counts())
            self.totals[r] += np.array(counts[-1], np.int64)
        return counts

    def step(self):
        for s in self.ranks:
            s.step(1)

    def step_partial(self, stage):
        for s in self.ranks:
            s.step_partial(stage)

    def iisph_step(self, min_iters=2):
        """SlabDriver.iisph_step with the all-reduce replaced by a sum over the contexts; returns the iteration count"""
        for s in self.ranks:
            s.iisph_predict()
        it, rho_avg = 0, self.real(0)
        while (float(rho_avg) - 1000.0) > 1.0 or it < min_iters:
            if it >= self.max_iters:
                self.truncated_steps += 1
                break
            tot, cnt = 0.0, 0
            for s in self.ranks:
                s_, c_ = s.iisph_iterate()
                tot += s_
                cnt += c_
            rho_avg = slab.mean_density(tot, cnt, self.real)
            it += 1
        for s in self.ranks:
            s.iisph_finish()
        self.last_iterations = it
        return it

    def union(self):
        """the owned particles of all ranks, concatenated in rank order: (pos, vel), for IISPH (pos, vel, pres).  Valid right after
        an exchange()."""
        parts = []
        for s in self.ranks:
            k = s.n_owned
            parts.append([a[:k] for a in s.download(pressure=self.iisph)])
        return tuple(np.concatenate([q[i] for q in parts]) for i in range(3 if self.iisph else 2))

    def close(self):
        for s in self.ranks:
            s.close()
        for b in self.send_l + self.send_r:
            if b is not None:
                b.free()
        self.ranks, self.send_l, self.send_r = [], [], []
