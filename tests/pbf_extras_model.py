"""Float64 restatement of the PBF tensile correction and vorticity confinement (DESIGN.md "PBF"), for the tests.

It extends tests/pbf_model.py and keeps its roundings: the cut-off tests, W and the spiky gradient round to float where the device
goes through the float helpers, everything else is plain float64, and the sums are formed in another order than the device's.
|omega| and |eta| are plain norms (the device forms them in SReal).  Both kernel sets (kernel_set, MULLER by default): W_q, s_corr and
the gradient of omega / eta follow the solver's W and pbf_grad.
"""
import numpy as np

from tests.pbf_model import pbf_grad, prototype_d
from tests.pcisph_model import MULLER, W, _len, _p, cut_margin, neighbourhood, pairs_within, real_of, sep, start_prediction

VORT_CUT = 1e-3   # N = 0 where |eta| <= VORT_CUT |omega| / h (a constant of the definition, not a setting)


def w_q(params, dq, kernel_set=MULLER):
    """W((dq h, 0, 0)), the reference value of s_corr"""
    h = _p(params, "interactionRadius")
    return float(W(params, np.array([[dq * h, 0.0, 0.0]]), kernel_set)[0])


def s_corr(params, d, k, dq, kernel_set=MULLER):
    """s_ij = -k (W(d) / W_q)^4, formed as r = W / W_q; r2 = r * r; -k * (r2 * r2)"""
    r = W(params, d, kernel_set) / w_q(params, dq, kernel_set)
    r2 = r * r
    return -k * (r2 * r2)


def pairs(params, x):
    """the step's neighbourhood: length(x_i - x_j) < h at the start positions, j != i"""
    return pairs_within(x, x, _p(params, "interactionRadius"), same=True)


def _bsum(idx, v, n):
    return np.stack([np.bincount(idx, v[:, a], n) for a in range(3)], axis=1)


def vorticity(params, xs, u, ii, jj, kernel_set=MULLER):
    """omega_i = sum_j (m / rho0) (u_i - u_j) x grad W_spiky(x*_i - x*_j) over the pairs (ii, jj) within h at x*"""
    m, rd, h = (_p(params, k) for k in ("particleMass", "restDensity", "interactionRadius"))
    d = xs[ii] - xs[jj]
    g = np.where((_len(d) < h)[:, None], (m / rd) * pbf_grad(params, d, kernel_set), 0.0)
    return _bsum(ii, np.cross(u[ii] - u[jj], g), len(xs))


def confinement(params, xs, omega, ii, jj, kernel_set=MULLER):
    """eta_i = sum_j (m / rho0) (|omega_j| - |omega_i|) grad W_spiky(x*_ij), and N_i (0 at or below the cut).  Returns (eta, N)."""
    m, rd, h = (_p(params, k) for k in ("particleMass", "restDensity", "interactionRadius"))
    w = np.linalg.norm(omega, axis=1)
    d = xs[ii] - xs[jj]
    g = np.where((_len(d) < h)[:, None], (m / rd) * pbf_grad(params, d, kernel_set), 0.0)
    eta = _bsum(ii, (w[jj] - w[ii])[:, None] * g, len(xs))
    en = np.linalg.norm(eta, axis=1)
    on = en > VORT_CUT * w / h
    N = np.where(on[:, None], eta / np.where(on, en, 1.0)[:, None], 0.0)
    return eta, N


def run(params, x, vel_adv, bpos=None, vb=None, eps=None, relaxation=0.01, min_iters=2, cap=50, eta=0.01, xsph=0.0, k=0.0, dq=0.2,
        eps_v=0.0, kernel_set=MULLER):
    """Steps 2-3 of a PBF step with s_corr (k > 0) and vorticity confinement (eps_v > 0); pbf_model.run otherwise.  Returns dict(iters,
    errors, lam, rho, dx, xs, vel, pos, eps, omega, eta_v, N, u, margin (pcisph_model.cut_margin over the pairs evaluated at predicted
    positions after the first iteration))."""
    x = np.asarray(x, np.float64)[:, :3]
    vel_adv = np.asarray(vel_adv, np.float64)[:, :3]
    m, rd, h, dt = (_p(params, kk) for kk in ("particleMass", "restDensity", "interactionRadius", "timestep"))
    if eps is None:
        eps = relaxation * prototype_d(params, kernel_set)[0]
    n = len(x)
    ii, jj, bi, bj = neighbourhood(params, x, bpos)
    if len(bi):
        bpos = np.asarray(bpos, np.float64)[:, :3]
        psi = rd * np.asarray(vb, np.float64)
    Wk = lambda d: W(params, d, kernel_set)            # noqa: E731
    Gk = lambda d: pbf_grad(params, d, kernel_set)     # noqa: E731
    real = real_of(params)
    xs = start_prediction(params, x, vel_adv)
    cap = min_iters if eta == 0 else cap
    errors = []
    l = 0
    margin = np.inf
    while True:
        # A: rho*, lambda, e
        d = sep(xs[ii], xs[jj], real)
        margin = cut_margin(d, h, margin) if l else margin   # (the first iteration's tests are the device's own)
        inside = _len(d) < h
        g = np.where(inside[:, None], (m / rd) * Gk(d), 0.0)
        rho = m * Wk(np.zeros((1, 3)))[0] + np.bincount(ii, np.where(inside, m * Wk(d), 0.0), n)
        gsum = _bsum(ii, g, n)
        gg = np.bincount(ii, np.sum(g * g, axis=1), n)
        gb = np.zeros((len(bi), 3))
        if len(bi):
            db = sep(xs[bi], bpos[bj], real)
            margin = cut_margin(db, h, margin) if l else margin
            insb = _len(db) < h
            gb = np.where(insb[:, None], (psi[bj] / rd)[:, None] * Gk(db), 0.0)
            rho = rho + np.bincount(bi, np.where(insb, psi[bj] * Wk(db), 0.0), n)
            gsum = gsum + _bsum(bi, gb, n)
        C = np.maximum(rho / rd - 1.0, 0.0)
        lam = -C / (np.sum(gsum * gsum, axis=1) + gg + eps)
        e = np.maximum(rho - rd, 0.0) / rd
        # B: dx with s_ij on the fluid pairs, the next predicted positions
        s = s_corr(params, d, k, dq, kernel_set) if k > 0 else 0.0
        dx = _bsum(ii, (lam[ii] + lam[jj] + s)[:, None] * g, n)
        if len(bi):
            dx = dx + _bsum(bi, lam[bi][:, None] * gb, n)
        xs = xs + dx
        l += 1
        errors.append(float(e.max()) if n else 0.0)
        if l >= cap or (eta > 0 and l >= min_iters and errors[-1] <= eta):
            break
    u = (xs - x) / dt
    vel = u.copy()
    d = sep(xs[ii], xs[jj], real)
    margin = cut_margin(d, h, margin)
    if xsph > 0:
        w = np.where(_len(d) < h, (m / rd) * Wk(d), 0.0)
        vel = vel + xsph * _bsum(ii, w[:, None] * (u[jj] - u[ii]), n)
    omega = eta_v = N = None
    if eps_v > 0:
        omega = vorticity(params, xs, u, ii, jj, kernel_set)
        eta_v, N = confinement(params, xs, omega, ii, jj, kernel_set)
        vel = vel + dt * eps_v * np.cross(N, omega)
    return dict(iters=l, errors=errors, lam=lam, rho=rho, dx=dx, xs=xs, vel=vel, pos=xs.copy(), eps=eps, omega=omega, eta_v=eta_v,
                N=N, u=u, margin=margin)
