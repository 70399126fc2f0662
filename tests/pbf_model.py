"""Float64 restatement of the PBF solve and integration (DESIGN.md "PBF"), for the tests.

Input is the device's own sorted start state of a step: the start positions x (NRS_ARR_SORTED_POS after the advection stage),
vel_adv (NRS_ARR_VEL_ADV) and the sorted boundary particles (NRS_ARR_B_SORTED, xyz + V_b).  Pairs are found by brute force.

As in tests/pcisph_model.py, the model rounds to float where the device goes through the float helpers of the reference (SURVEY
Q11): the cut-off tests, W (Wdefault), the spiky gradient (Wpressure_grad: float length, float kpress_grad and a float (h - |r|)^2
factor) and the first predicted position.  Everything else is plain float64, and the sums are formed in another order than the
device's.  Muller kernels only.
"""
import numpy as np

from tests.pcisph_model import F32, _len, _p, predict, w_dens


def spiky_grad(d, h, kpress_grad):
    """Wpressure_grad with the PBF guard: (float(kpress_grad) * (r / |r|)) * float((h - |r|)^2), 0 outside h and at |r| = 0"""
    d = np.asarray(d, np.float64)
    ln = _len(d).astype(np.float64)
    safe = np.where(ln > 0, ln, 1.0)
    c = ((h - ln) * (h - ln)).astype(F32).astype(np.float64)
    g = (float(F32(kpress_grad)) * (d / safe[..., None])) * c[..., None]
    return np.where(((ln * ln > h * h) | (ln == 0))[..., None], 0.0, g)


def prototype_d(params):
    """D_proto = |sum g|^2 + sum |g|^2 over the lattice points k s, 0 < |k s| < h, s = cbrt(m / rho0), g = (m / rho0) grad W_spiky(-k s)
    rounded to the build's precision.  Returns (D_proto, neighbours)."""
    double = np.asarray(params["particleMass"]).dtype == np.float64
    real = np.float64 if double else F32
    m, rd, h = (_p(params, k) for k in ("particleMass", "restDensity", "interactionRadius"))
    kpg = _p(params, "kpress_grad")
    s = float(real(np.cbrt(m / rd)))
    kmax = int(np.ceil(h / s)) + 1
    ks = np.arange(-kmax, kmax + 1)
    kz, ky, kx = np.meshgrid(ks, ks, ks, indexing="ij")
    k = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1).astype(np.float64)
    d = (-k * s).astype(real).astype(np.float64)
    keep = (_len(d) < h) & np.any(k != 0, axis=1)
    g = ((m / rd) * spiky_grad(d[keep], h, kpg)).astype(real).astype(np.float64)
    if len(g) == 0:
        return None, 0
    sg = g.sum(axis=0)
    return float(sg @ sg) + float(np.sum(g * g)), len(g)


def run(params, x, vel_adv, bpos=None, vb=None, eps=None, relaxation=0.01, min_iters=2, cap=50, eta=0.01, xsph=0.0):
    """Steps 2-3 of a PBF step.  eta = 0: exactly min_iters iterations.  Returns dict(iters, errors (max e after each iteration's
    launch A), lam, rho, dx, xs, vel, pos, eps)."""
    x = np.asarray(x, np.float64)[:, :3]
    vel_adv = np.asarray(vel_adv, np.float64)[:, :3]
    m, rd, h, dt = (_p(params, k) for k in ("particleMass", "restDensity", "interactionRadius", "timestep"))
    kp, kpg = _p(params, "kpoly"), _p(params, "kpress_grad")
    if eps is None:
        eps = relaxation * prototype_d(params)[0]
    n = len(x)
    # the step's neighbourhood: length(x_i - x_j) < h at the start positions, j != i
    ii, jj = np.nonzero(_len(x[:, None, :] - x[None, :, :]) < h)
    keep = ii != jj
    ii, jj = ii[keep], jj[keep]
    if bpos is not None and len(bpos):
        bpos = np.asarray(bpos, np.float64)[:, :3]
        psi = rd * np.asarray(vb, np.float64)
        bi, bj = np.nonzero(_len(x[:, None, :] - bpos[None, :, :]) < h)
    else:
        bpos, psi = np.zeros((0, 3)), np.zeros(0)
        bi = bj = np.zeros(0, np.int64)
    xs, _ = predict(x, vel_adv, np.zeros_like(x), dt, m)
    cap = min_iters if eta == 0 else cap
    errors = []
    l = 0

    def bsum(idx, v):
        return np.stack([np.bincount(idx, v[:, a], n) for a in range(3)], axis=1)

    while True:
        # A: rho*, lambda, e
        d = xs[ii] - xs[jj]
        inside = _len(d) < h
        g = np.where(inside[:, None], (m / rd) * spiky_grad(d, h, kpg), 0.0)
        rho = m * w_dens(np.zeros((1, 3)), h, kp)[0] + np.bincount(ii, np.where(inside, m * w_dens(d, h, kp), 0.0), n)
        gsum = bsum(ii, g)
        gg = np.bincount(ii, np.sum(g * g, axis=1), n)
        gb = np.zeros((len(bi), 3))
        if len(bi):
            db = xs[bi] - bpos[bj]
            insb = _len(db) < h
            gb = np.where(insb[:, None], (psi[bj] / rd)[:, None] * spiky_grad(db, h, kpg), 0.0)
            rho = rho + np.bincount(bi, np.where(insb, psi[bj] * w_dens(db, h, kp), 0.0), n)
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
        d = xs[ii] - xs[jj]
        w = np.where(_len(d) < h, (m / rd) * w_dens(d, h, kp), 0.0)
        vel = vel + xsph * bsum(ii, w[:, None] * (vel[jj] - vel[ii]))
    return dict(iters=l, errors=errors, lam=lam, rho=rho, dx=dx, xs=xs, vel=vel, pos=xs.copy(), eps=eps)
