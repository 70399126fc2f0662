"""Float64 restatement of the Akinci surface tension and wall adhesion (DESIGN.md "Akinci surface tension and adhesion"), for the tests.

Input is the device's own sorted start state of a step: the positions x (NRS_ARR_SORTED_POS), the densities rho (NRS_ARR_DENS) and the
sorted boundary particles (NRS_ARR_B_SORTED, xyz + V_b).  It keeps the roundings of tests/pcisph_model.py — length() is a float, the
separations are formed in the build's precision — and evaluates the two kernels C and A with the device's operations in the build's
precision (both have unbounded slope at the ends of their branches, where a radicand formed otherwise would not be the device's);
everything else is plain float64, and the sums are formed in another order than the device's.  Both kernel sets: the gradient of the
normals is the solver's W_grad.
"""
import numpy as np

from tests.pcisph_model import F32, MULLER, W, _len, _p, grad_W, neighbourhood, pairs_within, real_of, sep  # noqa: F401


def cakinci(d, h, ksurf1, ksurf2, real=np.float64):
    """Cakinci: ksurf1 (h - r)^3 r^3 for h / 2 < r <= h, ksurf1 (2 (h - r)^3 r^3 - ksurf2) for 0 < r <= h / 2, else 0; r = length(d) is
    a float, the rest is formed in `real`"""
    ln = _len(d).astype(real)
    h, k1, k2 = real(h), real(ksurf1), real(ksurf2)
    hr = h - ln
    with np.errstate(over="ignore", invalid="ignore"):
        a = (hr * hr * hr) * (ln * ln * ln)
        outer = k1 * a
        inner = k1 * (real(2) * (hr * hr * hr) * (ln * ln * ln) - k2)
    b1 = (2.0 * ln.astype(np.float64) > float(h)) & (ln <= h)
    b2 = (ln > 0) & (real(2) * ln <= h)
    return np.where(b1, outer, np.where(b2, inner, real(0))).astype(np.float64)


def aboundary_radicand(d, h, real=np.float64):
    """(in-branch mask, -4 r^2 / h + 6 r - 2 h as a float): the quotient in `real`, 6 r - 2 h in double and rounded to `real`"""
    ln = _len(d).astype(real)
    h = real(h)
    with np.errstate(over="ignore", invalid="ignore"):
        a = -((real(4) * (ln * ln)) / h)
        b = (6.0 * ln.astype(np.float64) - 2.0 * float(h)).astype(real)
        rad = (a + b).astype(F32)
    return (2.0 * ln.astype(np.float64) > float(h)) & (ln <= h), rad


def aboundary(d, h, bpol, real=np.float64, clamp=False):
    """Aboundary: bpol * (radicand)^(1/4) inside h / 2 < r <= h, else 0.  clamp=False: the reference's powf on a float, NaN where
    roundoff leaves the radicand negative; clamp=True: the force walk's form, the radicand clamped at 0 and the root as two correctly
    rounded float square roots"""
    inside, rad = aboundary_radicand(d, h, real)
    with np.errstate(invalid="ignore"):
        if clamp:
            res = np.sqrt(np.sqrt(np.where(rad > 0, rad, F32(0)).astype(F32)))
        else:
            res = np.power(rad, F32(0.25))
    return np.where(inside, real(bpol) * res.astype(real), real(0)).astype(np.float64)


def _bsum(idx, v, n):
    return np.stack([np.bincount(idx, v[:, a], n) for a in range(3)], axis=1)


def density(params, x, bpos=None, vb=None, kernel_set=MULLER):
    """the DENSITY stage: rho_i = m W(0) + sum_j m W(x_ij) + sum_b psi_b W(x_ib) over length < h (for scenes the device does not run)"""
    m, rd, h = (_p(params, k) for k in ("particleMass", "restDensity", "interactionRadius"))
    real = real_of(params)
    ii, jj, bi, bj = neighbourhood(params, x, bpos)
    x = np.asarray(x, np.float64)[:, :3]
    rho = m * W(params, np.zeros((1, 3)), kernel_set)[0] + np.bincount(ii, m * W(params, sep(x[ii], x[jj], real), kernel_set), len(x))
    if len(bi):
        b = np.asarray(bpos, np.float64)[:, :3]
        rho = rho + np.bincount(bi, rd * np.asarray(vb, np.float64)[bj] * W(params, sep(x[bi], b[bj], real), kernel_set), len(x))
    return rho


def normals(params, x, rho, ii, jj, kernel_set=MULLER):
    """n_i = h sum_j (m / rho_j) grad W(x_ij) over the fluid pairs (ii, jj)"""
    m, h = _p(params, "particleMass"), _p(params, "interactionRadius")
    d = sep(x[ii], x[jj], real_of(params))
    return h * _bsum(ii, (m / rho[jj])[:, None] * grad_W(params, d, kernel_set), len(x))


def run(params, x, rho, gamma, beta, bpos=None, vb=None, kernel_set=MULLER):
    """Returns dict(n, coh, curv, adh, f (their sum), ii, jj, bi, bj):
    coh = -gamma m m sum_j K_ij C(x_ij) x_ij / |x_ij|, curv = -gamma m sum_j K_ij (n_i - n_j), K_ij = 2 rho0 / (rho_i + rho_j), over the
    fluid pairs with length(x_ij) < h; adh = -beta m sum_b psi_b A(x_ib) x_ib / |x_ib| over the boundary particles (A's branch is the
    cut-off; the pairs are searched a little beyond h for that reason)."""
    x = np.asarray(x, np.float64)[:, :3]
    rho = np.asarray(rho, np.float64)
    m, rd, h = (_p(params, k) for k in ("particleMass", "restDensity", "interactionRadius"))
    k1, k2, bp = (_p(params, k) for k in ("ksurf1", "ksurf2", "bpol"))
    real = real_of(params)
    n = len(x)
    ii, jj, _, _ = neighbourhood(params, x, None)
    nrm = normals(params, x, rho, ii, jj, kernel_set)
    coh = np.zeros((n, 3))
    curv = np.zeros((n, 3))
    adh = np.zeros((n, 3))
    if gamma > 0:
        d = sep(x[ii], x[jj], real)
        K = 2.0 * rd / (rho[ii] + rho[jj])
        C = cakinci(d, h, k1, k2, real)
        ln = _len(d).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            u = d.astype(np.float64) / ln[:, None]
        coh = -gamma * m * m * _bsum(ii, np.where((C != 0)[:, None], (K * C)[:, None] * u, 0.0), n)
        curv = -gamma * m * _bsum(ii, K[:, None] * (nrm[ii] - nrm[jj]), n)
    bi = bj = np.zeros(0, np.int64)
    if beta > 0 and bpos is not None and len(bpos):
        b = np.asarray(bpos, np.float64)[:, :3]
        bi, bj = pairs_within(x, b, 1.01 * h, real=real)
        db = sep(x[bi], b[bj], real)
        A = aboundary(db, h, bp, real, clamp=True)
        ln = _len(db).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            u = db.astype(np.float64) / ln[:, None]
        psi = rd * np.asarray(vb, np.float64)[bj]
        adh = -beta * m * _bsum(bi, np.where((A != 0)[:, None], (psi * A)[:, None] * u, 0.0), n)
    return dict(n=nrm, coh=coh, curv=curv, adh=adh, f=coh + curv + adh, ii=ii, jj=jj, bi=bi, bj=bj)
