"""Float64 restatement of the DFSPH factor, the A/B launches, the warm start and both loops (DESIGN.md "DFSPH"), for the tests.

Input is the device's own sorted state of a step: the start positions x (NRS_ARR_SORTED_POS), the sorted velocities the divergence
solve starts from (NRS_ARR_SORTED_VEL after DENSITY), rho (NRS_ARR_DENS), the sorted boundary particles (NRS_ARR_B_SORTED, xyz +
V_b), vel_adv after P_ADVECT (NRS_ARR_VEL_ADV) and the sorted warm-start inputs K_prev (NRS_ARR_PRES after P_ADVECT) and Kv_prev
(NRS_ARR_DFSPH_KAPPA_V after DENSITY).  Pairs are found by brute force at the start positions, the only positions of the step.

As in tests/pbf_model.py, the model rounds to float where the device goes through the float helpers: the cut-off tests
and the gradient (pbf_model.pbf_grad).  The separations are formed in the build's precision.  Everything else is plain float64, with
the sums in another order than the device's.  Both kernel sets.
"""
import numpy as np

from tests.pbf_model import pbf_grad, prototype_d
from tests.pcisph_model import MULLER, W, _p, neighbourhood, real_of, sep

WARM = 0.5          # DFSPH_WARM: kappa = 0.5 K_prev / dt^2 in the warm-start pair
THRESHOLD = 1e-6    # alpha = 0 where D <= 1e-6 D_proto


class Pairs:
    """the step's neighbourhood with its gradients: g_ij = (m / rho0) pbf_grad(x_i - x_j), g_ib = (psi_b / rho0) pbf_grad(x_i - x_b)"""

    def __init__(self, params, x, bpos=None, vb=None, kernel_set=MULLER):
        real = real_of(params)
        self.n = n = len(x)
        x = np.asarray(x, np.float64)[:, :3]
        m, rd = _p(params, "particleMass"), _p(params, "restDensity")
        self.ii, self.jj, self.bi, self.bj = neighbourhood(params, x, bpos)
        self.g = (m / rd) * pbf_grad(params, sep(x[self.ii], x[self.jj], real), kernel_set) if len(self.ii) else np.zeros((0, 3))
        self.gb = np.zeros((0, 3))
        if len(self.bi):
            bpos = np.asarray(bpos, np.float64)[:, :3]
            psi = rd * np.asarray(vb, np.float64)
            self.gb = (psi[self.bj] / rd)[:, None] * pbf_grad(params, sep(x[self.bi], bpos[self.bj], real), kernel_set)

    def bsum(self, idx, v):
        return np.stack([np.bincount(idx, v[:, a], self.n) for a in range(3)], axis=1)


def density(params, x, bpos=None, vb=None, kernel_set=MULLER):
    """rho_i = m W(0) + sum_j m W(x_i - x_j) + sum_b psi_b W(x_i - x_b) over the step's neighbourhood (the density scan)"""
    real = real_of(params)
    x = np.asarray(x, np.float64)[:, :3]
    m, rd = _p(params, "particleMass"), _p(params, "restDensity")
    ii, jj, bi, bj = neighbourhood(params, x, bpos)
    rho = m * W(params, np.zeros((1, 3)), kernel_set)[0] + np.bincount(ii, m * W(params, sep(x[ii], x[jj], real), kernel_set), len(x))
    if len(bi):
        psi = rd * np.asarray(vb, np.float64)
        rho = rho + np.bincount(bi, psi[bj] * W(params, sep(x[bi], np.asarray(bpos)[bj, :3], real), kernel_set), len(x))
    return rho


def factor(params, pairs, kernel_set=MULLER):
    """alpha_i = 1 / D_i (0 where D_i <= 1e-6 D_proto), D_i = |sum_j g_ij + sum_b g_ib|^2 + sum_j |g_ij|^2.  Returns (alpha, D)."""
    gs = pairs.bsum(pairs.ii, pairs.g)
    if len(pairs.bi):
        gs = gs + pairs.bsum(pairs.bi, pairs.gb)
    D = np.sum(gs * gs, axis=1) + np.bincount(pairs.ii, np.sum(pairs.g * pairs.g, axis=1), pairs.n)
    thr = THRESHOLD * prototype_d(params, kernel_set)[0]
    with np.errstate(divide="ignore"):
        return np.where(D > thr, 1.0 / np.where(D > 0, D, 1.0), 0.0), D


def divergence(pairs, u):
    """div_i = sum_j (u_i - u_j) . g_ij + sum_b u_i . g_ib"""
    div = np.bincount(pairs.ii, np.sum((u[pairs.ii] - u[pairs.jj]) * pairs.g, axis=1), pairs.n)
    if len(pairs.bi):
        div = div + np.bincount(pairs.bi, np.sum(u[pairs.bi] * pairs.gb, axis=1), pairs.n)
    return div


def correction(pairs, kappa):
    """sum_j (kappa_i + kappa_j) g_ij + sum_b kappa_i g_ib"""
    s = pairs.bsum(pairs.ii, (kappa[pairs.ii] + kappa[pairs.jj])[:, None] * pairs.g)
    if len(pairs.bi):
        s = s + pairs.bsum(pairs.bi, kappa[pairs.bi][:, None] * pairs.gb)
    return s


def solve(params, pairs, alpha, u, K_prev=None, rho=None, min_iters=1, eta=0.0, cap=100, warm=True):
    """One DFSPH loop on the velocities u: the density solve when rho is given, else the divergence solve.  eta = 0: exactly
    min_iters iterations.  Returns dict(u, K, kappa, e (of the last iteration), rho_adv (density solve), iters, avgs, maxes (avg / max
    e of every iteration's A), first_e (e of the first A launch: the warm pair's, if any))."""
    dt, rd = _p(params, "timestep"), _p(params, "restDensity")
    u = np.asarray(u, np.float64)[:, :3].copy()
    n = pairs.n
    K_prev = np.zeros(n) if K_prev is None else np.asarray(K_prev, np.float64)

    def launch_a(u):
        div = divergence(pairs, u)
        if rho is None:
            return np.maximum(dt * div, 0.0), None
        ra = np.asarray(rho, np.float64) + (dt * rd) * div
        return np.maximum(ra - rd, 0.0) / rd, ra

    K = np.zeros(n)
    first_e = None
    if warm:
        e, _ = launch_a(u)
        first_e = e
        kappa = np.where(e > 0, WARM * K_prev / dt ** 2, 0.0)
        K = kappa * dt ** 2
        u = u - dt * correction(pairs, kappa)
    cap = min_iters if eta == 0 else cap
    l, avgs, maxes = 0, [], []
    while True:
        e, ra = launch_a(u)
        if first_e is None:
            first_e = e
        kappa = e * alpha / dt ** 2
        K = K + e * alpha
        u = u - dt * correction(pairs, kappa)
        l += 1
        avgs.append(float(e.mean()) if n else 0.0)
        maxes.append(float(e.max()) if n else 0.0)
        if l >= cap or (eta > 0 and l >= min_iters and avgs[-1] <= eta):
            break
    return dict(u=u, K=K, kappa=kappa, e=e, rho_adv=ra, iters=l, avgs=avgs, maxes=maxes, first_e=first_e)
