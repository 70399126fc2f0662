"""Float64 restatement of the implicit viscosity operator and its CG loop (DESIGN.md "Implicit viscosity"), for the tests.

Input is the device's own sorted state of a step: the start positions x (NRS_ARR_SORTED_POS), rho of the step's scan (NRS_ARR_DENS),
the sorted boundary particles (NRS_ARR_B_SORTED, xyz + V_b) and b = vel_adv after P_ADVECT of a twin context with the solve off.

  (A u)_i = u_i - dt nu   (rho0 / rho_i) 10 sum_j (rho0 / rho_j) ((u_i - u_j) . x_ij) / (|x_ij|^2 + 0.01 h^2) g_ij
                - dt nu_b (rho0 / rho_i) 10 sum_b                ( u_i        . x_ib) / (|x_ib|^2 + 0.01 h^2) g_ib

on dfsph_model.Pairs, whose neighbourhood and gradients round to float where the device goes through the float helpers; the
separations are formed in the build's precision.  Everything else is plain float64 (or, with real=np.float32 in cg(), float32 vectors
with double dot products, as the device's fp32 build), with the sums in another order than the device's.
"""
import numpy as np

from tests.dfsph_model import Pairs
from tests.pcisph_model import MULLER, _p, real_of, sep


class Operator:
    def __init__(self, params, x, rho, nu, nu_b=0.0, bpos=None, vb=None, kernel_set=MULLER, pairs=None):
        real = real_of(params)
        x = np.asarray(x, np.float64)[:, :3]
        self.n = len(x)
        self.pairs = pr = pairs if pairs is not None else Pairs(params, x, bpos, vb, kernel_set)
        h, rd, dt = _p(params, "interactionRadius"), _p(params, "restDensity"), _p(params, "timestep")
        rho = np.asarray(rho, np.float64)
        s = rd / rho
        eps = 0.01 * h * h
        self.d = sep(x[pr.ii], x[pr.jj], real) if len(pr.ii) else np.zeros((0, 3))
        # w_ij: the fluid pair's scalar weight, symmetric in i and j; the block of the pair is w_ij g_ij x_ij^T
        self.w = 10.0 * dt * nu * s[pr.ii] * s[pr.jj] / (np.sum(self.d * self.d, axis=1) + eps)
        self.db = np.zeros((0, 3))
        self.wb = np.zeros(0)
        if len(pr.bi) and nu_b > 0:
            self.db = sep(x[pr.bi], np.asarray(bpos, np.float64)[pr.bj, :3], real)
            self.wb = 10.0 * dt * nu_b * s[pr.bi] / (np.sum(self.db * self.db, axis=1) + eps)

    def apply(self, u):
        pr = self.pairs
        u = np.asarray(u, np.float64)
        out = u.copy()
        if len(pr.ii):
            c = self.w * np.sum((u[pr.ii] - u[pr.jj]) * self.d, axis=1)
            out -= pr.bsum(pr.ii, c[:, None] * pr.g)
        if len(self.wb):
            c = self.wb * np.sum(u[pr.bi] * self.db, axis=1)
            out -= pr.bsum(pr.bi, c[:, None] * pr.gb)
        return out

    def matrix(self):
        """the assembled 3n x 3n matrix (scipy.sparse.csr_matrix)"""
        import scipy.sparse as sp

        pr, n = self.pairs, self.n
        rows, cols, vals = [np.arange(3 * n)], [np.arange(3 * n)], [np.ones(3 * n)]
        for a in range(3):
            for b in range(3):
                if len(pr.ii):
                    blk = self.w * pr.g[:, a] * self.d[:, b]   # -(blk) u_i + blk u_j
                    rows += [3 * pr.ii + a, 3 * pr.ii + a]
                    cols += [3 * pr.ii + b, 3 * pr.jj + b]
                    vals += [-blk, blk]
                if len(self.wb):
                    blk = self.wb * pr.gb[:, a] * self.db[:, b]
                    rows.append(3 * pr.bi + a)
                    cols.append(3 * pr.bi + b)
                    vals.append(-blk)
        return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(3 * n, 3 * n))


def alpha_of(rr, pq):
    return rr / pq if pq > 0.0 else 0.0


def beta_of(rr_new, rr):
    return rr_new / rr if rr > 0.0 else 0.0


def cg(op, b, tol=0.0, min_iters=1, max_iters=0, real=np.float64):
    """plain CG from u0 = b under the exit rule: stop after iteration l >= min_iters with rr <= tol^2 bb, or at max_iters (0 = 100);
    tol = 0: exactly min_iters iterations.  `iters` counts the iterations that began with rr > 0; `queued` all of them.
    real=np.float32: vectors and per-particle terms in float32, dot products summed in double."""
    R = real
    f = lambda v: np.asarray(v, R)
    dot = lambda a, c: float(np.sum(np.sum(f(a) * f(c), axis=1, dtype=R).astype(np.float64)))
    b = f(np.asarray(b, np.float64)[:, :3])
    u = b.copy()
    r = f(b - f(op.apply(b)))
    p = r.copy()
    rr, bb = dot(r, r), dot(b, b)
    cap = min_iters if tol == 0 else (max_iters or 100)
    l = counted = 0
    hist = [rr]
    while True:
        q = f(op.apply(p))
        a = alpha_of(rr, dot(p, q))
        if rr > 0.0:
            counted += 1
        if a != 0.0:
            u = f(u + R(a) * p)
            r = f(r - R(a) * q)
        rr_new = dot(r, r)
        p = f(r + R(beta_of(rr_new, rr)) * p)
        rr = rr_new
        hist.append(rr)
        l += 1
        if l >= cap or (tol > 0 and l >= min_iters and rr <= tol * tol * bb):
            break
    return dict(u=np.asarray(u, np.float64), iters=counted, queued=l, residual=np.sqrt(rr), rhs_norm=np.sqrt(bb), rr=hist)
