"""Float64 restatement of the PBF solve and integration (DESIGN.md "PBF"), for the tests.

Input is the device's own sorted start state of a step: the start positions x (NRS_ARR_SORTED_POS after the advection stage),
vel_adv (NRS_ARR_VEL_ADV) and the sorted boundary particles (NRS_ARR_B_SORTED, xyz + V_b).  Pairs are found by brute force.

As in tests/pcisph_model.py, the model rounds to float where the device goes through the float helpers of the reference (SURVEY
Q11): the cut-off tests, W (Wdefault), the spiky gradient (Wpressure_grad: float length, float kpress_grad and a float (h - |r|)^2
factor) and the first predicted position.  Everything else is plain float64, and the sums are formed in another order than the
device's.  Both kernel sets: for Monaghan, W and the gradient are pcisph_model's Monaghan restatement (pbf_grad), with the
loop's cut-off at h on top of the 2h support.
"""
import numpy as np

from tests.pcisph_model import F32, MULLER, W, _len, _p, lattice, neighbourhood, real_of, sep, start_prediction, w_monaghan_grad


def spiky_grad(d, h, kpress_grad, real=np.float64):
    """Wpressure_grad with the PBF guard, in the build's precision: (float(kpress_grad) * (r / |r|)) * float((h - |r|)^2), 0 outside h
    (|r|^2 > h^2) and where the float length |r| is 0"""
    ln = _len(d).astype(real)
    d = np.asarray(d).astype(real)
    safe = np.where(ln > 0, ln, real(1))
    hl = real(h) - ln
    c = (hl * hl).astype(F32).astype(real)
    with np.errstate(over="ignore", invalid="ignore"):
        g = (real(F32(kpress_grad)) * (d / safe[..., None])) * c[..., None]
    out = (ln * ln > real(h) * real(h)) | (ln == 0)
    return np.where(out[..., None], real(0), g).astype(np.float64)


def pbf_grad(params, d, kernel_set=MULLER):
    """the PBF gradient (pbf_grad): Wpressure_grad for the Muller set, Monaghan's W_grad for Monaghan, 0 at zero separation; without
    the loop's cut-off at h (Monaghan's own support is 2h)"""
    h = _p(params, "interactionRadius")
    if kernel_set == MULLER:
        return spiky_grad(d, h, _p(params, "kpress_grad"), real_of(params))
    g = w_monaghan_grad(d, h, real_of(params)).astype(np.float64)
    return np.where((_len(d) == 0)[..., None], 0.0, g)


def prototype_d(params, kernel_set=MULLER):
    """D_proto = |sum g|^2 + sum |g|^2 over the lattice points k s, 0 < |k s| < h, s = cbrt(m / rho0), g = (m / rho0) pbf_grad(-k s)
    rounded to the build's precision.  Returns (D_proto, neighbours)."""
    real = real_of(params)
    m, rd = _p(params, "particleMass"), _p(params, "restDensity")
    g = ((m / rd) * pbf_grad(params, lattice(params), kernel_set)).astype(real).astype(np.float64)
    if len(g) == 0:
        return None, 0
    sg = g.sum(axis=0)
    return float(sg @ sg) + float(np.sum(g * g)), len(g)


def run(params, x, vel_adv, bpos=None, vb=None, eps=None, relaxation=0.01, min_iters=2, cap=50, eta=0.01, xsph=0.0, kernel_set=MULLER):
    """Steps 2-3 of a PBF step.  eta = 0: exactly min_iters iterations.  Returns dict(iters, errors (max e after each iteration's
    launch A), lam, rho, dx, xs, vel, pos, eps)."""
    x = np.asarray(x, np.float64)[:, :3]
    vel_adv = np.asarray(vel_adv, np.float64)[:, :3]
    m, rd, h, dt = (_p(params, k) for k in ("particleMass", "restDensity", "interactionRadius", "timestep"))
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

    def bsum(idx, v):
        return np.stack([np.bincount(idx, v[:, a], n) for a in range(3)], axis=1)

    while True:
        # A: rho*, lambda, e
        d = sep(xs[ii], xs[jj], real)
        inside = _len(d) < h
        g = np.where(inside[:, None], (m / rd) * Gk(d), 0.0)
        rho = m * Wk(np.zeros((1, 3)))[0] + np.bincount(ii, np.where(inside, m * Wk(d), 0.0), n)
        gsum = bsum(ii, g)
        gg = np.bincount(ii, np.sum(g * g, axis=1), n)
        gb = np.zeros((len(bi), 3))
        if len(bi):
            db = sep(xs[bi], bpos[bj], real)
            insb = _len(db) < h
            gb = np.where(insb[:, None], (psi[bj] / rd)[:, None] * Gk(db), 0.0)
            rho = rho + np.bincount(bi, np.where(insb, psi[bj] * Wk(db), 0.0), n)
            gsum = gsum + bsum(bi, gb)
        C = np.maximum(rho / rd - 1.0, 0.0)
        lam = -C / (np.sum(gsum * gsum, axis=1) + gg + eps)
        e = np.maximum(rho - rd, 0.0) / rd
        # B: dx, the next predicted positions
        dx = bsum(ii, (lam[ii] + lam[jj])[:, None] * g)
        if len(bi):
            dx = dx + bsum(bi, lam[bi][:, None] * gb)
        xs = xs + dx
        l += 1
        errors.append(float(e.max()) if n else 0.0)
        if l >= cap or (eta > 0 and l >= min_iters and errors[-1] <= eta):
            break
    vel = (xs - x) / dt
    if xsph > 0:
        d = sep(xs[ii], xs[jj], real)
        w = np.where(_len(d) < h, (m / rd) * Wk(d), 0.0)
        vel = vel + xsph * bsum(ii, w[:, None] * (vel[jj] - vel[ii]))
    return dict(iters=l, errors=errors, lam=lam, rho=rho, dx=dx, xs=xs, vel=vel, pos=xs.copy(), eps=eps)
