"""Float64 restatement of the PCISPH loop and integration (DESIGN.md "PCISPH"), for the tests.

Input is the device's own sorted start state of a step: the start positions x (NRS_ARR_SORTED_POS after the advection stage),
vel_adv (NRS_ARR_VEL_ADV) and the sorted boundary particles (NRS_ARR_B_SORTED, xyz + V_b).  Pairs are found by brute force, in
row chunks (pairs_within).

The device's vector helpers follow the reference's: dot() and length() return float, and the scalar operand of a
scalar-vector product is a float, also in the fp64 build.  Where the definition goes through those helpers — the cut-off tests,
W_dens / W_grad and the position prediction of k_iisph_integrate — the model rounds to float at the same places; everything else is
plain float64.  The sums are formed in another order than the device's, which costs a few units in the last place of fp64.
The separations of the cut-off tests and kernels, and the first predicted positions x*0, are formed in the build's precision: from the
device's own start state the model's first cut-off decisions are the device's.

Both kernel sets (kernel_set=MULLER, the default, or MONAGHAN).  The Monaghan cubic spline is restated with the device's roundings
(nrs_math.h Wmonaghan / Wmonaghan_grad): length() in float, the constants evaluated in double and rounded to the build's precision,
the rest in that precision.  Its support is 2h, but the loop's cut-off is h (length < h), applied on top.  W_grad at r = 0 is NaN
for Monaghan (0 / 0): the model gives the same NaN for a coincident fluid pair, as the device does; the tests' scenes hold none.
"""
import numpy as np

F32 = np.float32
MONAGHAN, MULLER = 0, 1   # NRS_KERNEL_SET_*


def _p(params, name):
    return float(np.asarray(params[name]).reshape(-1)[0])


def real_of(params):
    """the build's precision of a parameter block"""
    return np.float64 if np.asarray(params["particleMass"]).dtype == np.float64 else F32


def _len(d):
    """length() of the device: float of the dot product, formed in the operands' precision (float32 for float32 operands)"""
    d = np.asarray(d)
    if d.dtype != F32:
        d = d.astype(np.float64)
    dot = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(F32)
    return np.sqrt(dot)


def pairs_within(x, y, h, same=False, rows=None, real=np.float64):
    """(i, j) with length(x_i - y_j) < h, the difference formed in `real`, sorted by i then j (j != i when same): a brute-force search
    in row chunks, so that a few thousand particles need no n x n x 3 array"""
    x, y = np.asarray(x)[:, :3].astype(real), np.asarray(y)[:, :3].astype(real)
    rows = rows or max(1, 2_000_000 // max(1, len(y)))
    out_i, out_j = [], []
    for a in range(0, len(x), rows):
        i, j = np.nonzero(_len(x[a:a + rows, None, :] - y[None, :, :]) < h)
        i = i + a
        if same:
            keep = i != j
            i, j = i[keep], j[keep]
        out_i.append(i)
        out_j.append(j)
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(out_i), np.concatenate(out_j)


def w_dens(d, h, kpoly, real=np.float64):
    """Wdefault (poly6) in the build's precision `real`: r2 = length * length (a float product), h2 = h * h, kpoly * (h2 - r2)^3 with
    the cube formed in double and rounded once"""
    ln = _len(d)
    r2 = (ln * ln).astype(real)
    h2 = real(h) * real(h)
    c = (h2 - r2).astype(np.float64)
    with np.errstate(over="ignore"):
        b = (c * c * c).astype(real)
    return np.where(r2 > h2, real(0), real(kpoly) * b).astype(np.float64)


def w_grad(d, h, kpoly_grad, real=np.float64):
    """Wdefault_grad in the build's precision: (float(kpoly_grad) * r) * float((h2 - r2)^2 in float)"""
    ln = _len(d)
    d = np.asarray(d).astype(real)
    r2 = (ln * ln).astype(real)
    h2 = real(h) * real(h)
    with np.errstate(over="ignore", invalid="ignore"):
        f = (h2 - r2).astype(F32)
        b = (f * f).astype(real)
        g = (real(F32(kpoly_grad)) * d) * b[..., None]
    return np.where((r2 > h2)[..., None], real(0), g).astype(np.float64)


def _monaghan_consts(h, real):
    """invH = (R)(1 / h) and the normalisation (R)(1 / (4 pi h^3)), both evaluated in double as the device does"""
    hd = float(real(h))
    return real(1.0 / hd), real(1.0 / (4.0 * 3.14159265358979323846 * hd * hd * hd))


def w_monaghan(d, h, real=np.float64):
    """Wmonaghan (support 2h, no cut-off at h): q = length * invH; m_v ((2 - q)^3 - 4 (1 - q)^3) for q < 1, m_v (2 - q)^3 for q < 2,
    else 0, in the build's precision `real`"""
    inv_h, m_v = _monaghan_consts(h, real)
    q = _len(d).astype(real) * inv_h
    one, two, four = real(1), real(2), real(4)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = two - q, one - q
        v1 = m_v * (a * a * a - four * b * b * b)
        v2 = m_v * (a * a * a)
    return np.where((q >= 0) & (q < 1), v1, np.where((q >= 1) & (q < 2), v2, real(0)))


def w_monaghan_grad(d, h, real=np.float64):
    """Wmonaghan_grad (support 2h): float(m_g invH s / dist) * r for q < 1 (s = -3 (2 - q)^2 + 12 (1 - q)^2), float(m_g s invH / dist)
    * r for q < 2 (s = -3 (2 - q)^2), else 0; NaN at r = 0 (0 / 0)"""
    d = np.asarray(d)
    dr = d.astype(real)
    inv_h, m_g = _monaghan_consts(h, real)
    dist = _len(d).astype(real)
    q = dist * inv_h
    one, two = real(1), real(2)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a, b = two - q, one - q
        s1 = real(-3) * a * a
        s1 = s1 + real(12) * b * b
        c1 = m_g * inv_h * s1 / dist
        s2 = real(-3) * a * a
        c2 = m_g * s2 * inv_h / dist
        b1, b2 = (q >= 0) & (q < 1), (q >= 1) & (q < 2)
        c = np.where(b1, c1, np.where(b2, c2, real(0))).astype(F32).astype(real)   # (the float scalar of scalar * vector)
        g = c[..., None] * dr
    return np.where((b1 | b2)[..., None], g, real(0))


def W(params, d, kernel_set=MULLER):
    """the solvers' W_dens (without their cut-off at h): Wdefault or Wmonaghan"""
    h = _p(params, "interactionRadius")
    if kernel_set == MULLER:
        return w_dens(d, h, _p(params, "kpoly"))
    return w_monaghan(d, h, real_of(params)).astype(np.float64)


def grad_W(params, d, kernel_set=MULLER):
    """the solvers' W_grad (without their cut-off at h): Wdefault_grad or Wmonaghan_grad (NaN at r = 0)"""
    h = _p(params, "interactionRadius")
    if kernel_set == MULLER:
        return w_grad(d, h, _p(params, "kpoly_grad"))
    return w_monaghan_grad(d, h, real_of(params)).astype(np.float64)


def predict(x, vel_adv, fp, dt, m):
    """x + dt (vel_adv + dt Fp / m) with the float scalar operands of k_iisph_integrate"""
    dtf, mf = float(F32(dt)), float(F32(m))
    v = vel_adv + (dtf * fp) / mf
    return x + dtf * v, v


def lattice(params, spacing=0.0):
    """the prototype's lattice neighbours: the separations -k s (k in Z^3, 0 < length(k s) < h) in the build's precision, as float64;
    spacing 0 = cbrt(m / rho0)"""
    real = real_of(params)
    m, rd, h = (_p(params, k) for k in ("particleMass", "restDensity", "interactionRadius"))
    s = float(real(spacing if spacing > 0 else np.cbrt(m / rd)))
    kmax = int(np.ceil(h / s)) + 1
    ks = np.arange(-kmax, kmax + 1)
    kz, ky, kx = np.meshgrid(ks, ks, ks, indexing="ij")
    k = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1).astype(np.float64)
    d = (-k * s).astype(real)
    keep = (_len(d) < h) & np.any(k != 0, axis=1)
    return d[keep].astype(np.float64)


def prototype_delta(params, spacing=0.0, kernel_set=MULLER):
    """delta = -1 / (beta (-sum g . sum g - sum g . g)), beta = 2 (dt m / rho0)^2, over the lattice points k s, 0 < |k s| < h,
    g = W_grad(-k s); spacing 0 = cbrt(m / rho0).  Returns (delta, neighbours)."""
    real = real_of(params)
    m, rd, dt = (_p(params, k) for k in ("particleMass", "restDensity", "timestep"))
    d = lattice(params, spacing)
    g = grad_W(params, d, kernel_set).astype(real).astype(np.float64)
    if len(g) == 0:
        return None, 0
    sg = g.sum(axis=0)
    gg = float(np.sum(g * g))
    beta = 2.0 * (dt * m / rd) ** 2
    return -1.0 / (beta * (-float(sg @ sg) - gg)), len(g)


def cut_margin(d, h, margin=np.inf):
    """min over the separations d of |length(d) / h - 1| (and `margin`): how close a pair comes to the cut-off h"""
    return min(margin, float(np.min(np.abs(_len(d) / h - 1.0), initial=np.inf)))


def sep(a, b, real):
    """a - b formed in the build's precision, as the device forms the separations of its cut-off tests and kernels"""
    return np.asarray(a).astype(real) - np.asarray(b).astype(real)


def start_prediction(params, x, vel_adv):
    """x*0 = x + dt vel_adv in the build's precision, with the float dt of the device's scalar * vector (pci_predict with Fp = 0): for
    the device's own start state the model's first cut-off decisions are then the device's"""
    real = real_of(params)
    dtf = real(F32(_p(params, "timestep")))
    return (np.asarray(x).astype(real) + dtf * np.asarray(vel_adv).astype(real)).astype(np.float64)


def neighbourhood(params, x, bpos=None):
    """the step's neighbourhood at the start positions: fluid pairs (ii, jj), j != i, and fluid-boundary pairs (bi, bj), all with
    length < h"""
    h, real = _p(params, "interactionRadius"), real_of(params)
    ii, jj = pairs_within(x, x, h, same=True, real=real)
    if bpos is not None and len(bpos):
        bi, bj = pairs_within(x, bpos, h, real=real)
    else:
        bi = bj = np.zeros(0, np.int64)
    return ii, jj, bi, bj


def run(params, x, vel_adv, bpos=None, vb=None, delta=None, min_iters=3, cap=50, eta=0.01, kernel_set=MULLER):
    """Steps 3-4 of a PCISPH step.  Returns dict(iters, errors (max e after each iteration), p, rho, fp, fp_boundary (the boundary
    particles' share of fp), near_boundary (start-position neighbourhood holds a boundary particle), xs, vel, pos, margin (cut_margin
    over the pairs the loop evaluated at predicted positions after the first iteration))."""
    x = np.asarray(x, np.float64)[:, :3]
    vel_adv = np.asarray(vel_adv, np.float64)[:, :3]
    m, rd, h, dt = (_p(params, k) for k in ("particleMass", "restDensity", "interactionRadius", "timestep"))
    if delta is None:
        delta = prototype_delta(params, kernel_set=kernel_set)[0]
    n = len(x)
    ii, jj, bi, bj = neighbourhood(params, x, bpos)
    if len(bi):
        bpos = np.asarray(bpos, np.float64)[:, :3]
        psi = rd * np.asarray(vb, np.float64)
    Wk = lambda d: W(params, d, kernel_set)          # noqa: E731
    Gk = lambda d: grad_W(params, d, kernel_set)     # noqa: E731
    real = real_of(params)
    xs = start_prediction(params, x, vel_adv)
    p = np.zeros(n)
    fp = np.zeros_like(x)
    errors = []
    l = 0
    margin = np.inf
    with np.errstate(invalid="ignore"):   # (a coincident pair gives Monaghan's NaN gradient, as on the device)
        while True:
            # A: predicted density, pressure, error
            d = sep(xs[ii], xs[jj], real)
            margin = cut_margin(d, h, margin) if l else margin   # (the first iteration's tests are the device's own)
            w = np.where(_len(d) < h, m * Wk(d), 0.0)
            rho = m * Wk(np.zeros((1, 3)))[0] + np.bincount(ii, w, n)
            if len(bi):
                db = sep(xs[bi], bpos[bj], real)
                margin = cut_margin(db, h, margin) if l else margin
                wb = np.where(_len(db) < h, psi[bj] * Wk(db), 0.0)
                rho = rho + np.bincount(bi, wb, n)
            p = np.maximum(p + delta * (rho - rd), 0.0)
            e = np.maximum(rho - rd, 0.0) / rd
            # B: pressure force, next predicted positions
            g = np.where((_len(d) < h)[:, None], Gk(d), 0.0)
            c = -(m * m) * ((p[ii] + p[jj]) / (rd * rd))
            fp = np.stack([np.bincount(ii, c * g[:, a], n) for a in range(3)], axis=1)
            fpb = np.zeros_like(fp)
            if len(bi):
                gb = np.where((_len(db) < h)[:, None], Gk(db), 0.0)
                cb = -(m * psi[bj]) * (p[bi] / (rd * rd))
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
                delta=delta, margin=margin)
