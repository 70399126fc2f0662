"""Float64 restatement of the PCISPH loop and integration (DESIGN.md "PCISPH"), for the tests.

Input is the device's own sorted start state of a step: the start positions x (NRS_ARR_SORTED_POS after the advection stage),
vel_adv (NRS_ARR_VEL_ADV) and the sorted boundary particles (NRS_ARR_B_SORTED, xyz + V_b).  Pairs are found by brute force.

The device's vector helpers follow the reference's: dot() and length() return float, and the scalar operand of a
scalar-vector product is a float, also in the fp64 build.  Where the definition goes through those helpers — the cut-off tests,
W_dens / W_grad and the position prediction of k_iisph_integrate — the model rounds to float at the same places; everything else is
plain float64.  The sums are formed in another order than the device's, which costs a few units in the last place of fp64.
"""
import numpy as np

F32 = np.float32


def _p(params, name):
    return float(np.asarray(params[name]).reshape(-1)[0])


def _len(d):
    """length() of the device: float of the float-valued dot product"""
    d = np.asarray(d, np.float64)
    dot = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(F32)
    return np.sqrt(dot)


def w_dens(d, h, kpoly):
    """Wdefault (poly6): r2 = length * length in float, (h2 - r2)^3 in double"""
    ln = _len(d)
    r2 = (ln * ln).astype(np.float64)
    h2 = h * h
    b = (h2 - r2) ** 3
    return np.where(r2 > h2, 0.0, kpoly * b)


def w_grad(d, h, kpoly_grad):
    """Wdefault_grad: (float(kpoly_grad) * r) * float((h2 - r2)^2 in float)"""
    d = np.asarray(d, np.float64)
    ln = _len(d)
    r2 = (ln * ln).astype(np.float64)
    h2 = h * h
    f = (h2 - r2).astype(F32)
    b = (f * f).astype(np.float64)
    g = (float(F32(kpoly_grad)) * d) * b[..., None]
    return np.where((r2 > h2)[..., None], 0.0, g)


def predict(x, vel_adv, fp, dt, m):
    """x + dt (vel_adv + dt Fp / m) with the float scalar operands of k_iisph_integrate"""
    dtf, mf = float(F32(dt)), float(F32(m))
    v = vel_adv + (dtf * fp) / mf
    return x + dtf * v, v


def prototype_delta(params, spacing=0.0):
    """delta = -1 / (beta (-sum g . sum g - sum g . g)), beta = 2 (dt m / rho0)^2, over the lattice points k s, 0 < |k s| < h,
    g = W_grad(-k s); spacing 0 = cbrt(m / rho0).  Returns (delta, neighbours)."""
    double = np.asarray(params["particleMass"]).dtype == np.float64
    real = np.float64 if double else F32
    m, rd, h, dt = (_p(params, k) for k in ("particleMass", "restDensity", "interactionRadius", "timestep"))
    kpg = _p(params, "kpoly_grad")
    s = float(real(spacing if spacing > 0 else np.cbrt(m / rd)))
    kmax = int(np.ceil(h / s)) + 1
    ks = np.arange(-kmax, kmax + 1)
    kz, ky, kx = np.meshgrid(ks, ks, ks, indexing="ij")
    k = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1).astype(np.float64)
    d = (-k * s).astype(real).astype(np.float64)
    keep = (_len(d) < h) & np.any(k != 0, axis=1)
    g = w_grad(d[keep], h, kpg).astype(real).astype(np.float64)
    if len(g) == 0:
        return None, 0
    sg = g.sum(axis=0)
    gg = float(np.sum(g * g))
    beta = 2.0 * (dt * m / rd) ** 2
    return -1.0 / (beta * (-float(sg @ sg) - gg)), len(g)


def run(params, x, vel_adv, bpos=None, vb=None, delta=None, min_iters=3, cap=50, eta=0.01):
    """Steps 3-4 of a PCISPH step.  Returns dict(iters, errors (max e after each iteration), p, rho, fp, fp_boundary (the boundary
    particles' share of fp), near_boundary (start-position neighbourhood holds a boundary particle), xs, vel, pos)."""
    x = np.asarray(x, np.float64)[:, :3]
    vel_adv = np.asarray(vel_adv, np.float64)[:, :3]
    m, rd, h, dt = (_p(params, k) for k in ("particleMass", "restDensity", "interactionRadius", "timestep"))
    kp, kpg = _p(params, "kpoly"), _p(params, "kpoly_grad")
    if delta is None:
        delta = prototype_delta(params)[0]
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
    p = np.zeros(n)
    fp = np.zeros_like(x)
    errors = []
    l = 0
    while True:
        # A: predicted density, pressure, error
        d = xs[ii] - xs[jj]
        w = np.where(_len(d) < h, m * w_dens(d, h, kp), 0.0)
        rho = m * w_dens(np.zeros((1, 3)), h, kp)[0] + np.bincount(ii, w, n)
        if len(bi):
            db = xs[bi] - bpos[bj]
            wb = np.where(_len(db) < h, psi[bj] * w_dens(db, h, kp), 0.0)
            rho = rho + np.bincount(bi, wb, n)
        p = np.maximum(p + delta * (rho - rd), 0.0)
        e = np.maximum(rho - rd, 0.0) / rd
        # B: pressure force, next predicted positions
        g = w_grad(d, h, kpg)
        c = np.where(_len(d) < h, -(m * m) * ((p[ii] + p[jj]) / (rd * rd)), 0.0)
        fp = np.stack([np.bincount(ii, c * g[:, a], n) for a in range(3)], axis=1)
        fpb = np.zeros_like(fp)
        if len(bi):
            gb = w_grad(db, h, kpg)
            cb = np.where(_len(db) < h, -(m * psi[bj]) * (p[bi] / (rd * rd)), 0.0)
            fpb = np.stack([np.bincount(bi, cb * gb[:, a], n) for a in range(3)], axis=1)
            fp = fp + fpb
        xs, _ = predict(x, vel_adv, fp, dt, m)
        l += 1
        errors.append(float(e.max()) if n else 0.0)
        if l >= cap or (l >= min_iters and errors[-1] <= eta):
            break
    pos, vel = predict(x, vel_adv, fp, dt, m)
    near = np.zeros(n, bool)
    near[bi] = True
    return dict(iters=l, errors=errors, p=p, rho=rho, fp=fp, fp_boundary=fpb, near_boundary=near, xs=xs, vel=vel, pos=pos,
                delta=delta)
