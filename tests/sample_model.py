"""Brute-force numpy model of the field sampler (include/nereus_hip.h "field sampling"; DESIGN.md "Field sampling"), for the tests.

Input is the state the device samples: the downloaded positions and velocities, the query positions in the build's precision and,
for the wall term, the sorted boundary array (NRS_ARR_B_SORTED, xyz + V_b).  Neighbours are found by brute force
(pcisph_model.pairs_within: the difference in the build's precision, the float length() of the device); every TERM is formed as the
device forms it, in the build's precision `real`, with the smoothing kernels of pcisph_model (pinned to the reference by
test_model_kernels_pin.py):

    density    m * W(d)                        (real)      wall: (restDensity * V_b) * W(d)
    gradient   float(m) * grad W(d)            (the float scalar operand of scalar x vector); dropped where length(d) == 0
    velocity   float(m * W(d)) * v_j           numerator; the denominator is the fluid-only density sum

and the terms are summed in float64.  So the model differs from the device only by the rounding of a sum of k terms in `real`.

Tolerance (derived, not tuned).  A sequential sum of k terms t_1..t_k in a format with unit roundoff u = eps / 2 is off by at most
gamma_(k-1) * A with A = sum |t_i| and gamma_n = n u / (1 - n u); k * eps * A is that bound with a factor two of slack:

    |device - model| <= k * eps * A                                          for the density and each gradient component,

and for the velocity v = N / D, with bN = k eps A_N the bound of the numerator component and bD = k eps D that of the denominator
(all its terms are >= 0, so A_D = D):

    |device - v| <= (bN + |v| bD) / (D - bD) * (1 + eps / 2) + (eps / 2) |v|

(the quotient of the two perturbed sums, then the one rounding of the division); its w component, the denominator, is within bD.
Counts, and with them the cut-off decisions, are exact.
"""
import numpy as np

from tests import pcisph_model as pm

F32 = np.float32
DENSITY, GRADIENT, VELOCITY, COUNT, WALLS = 1, 2, 4, 8, 16


def lattice_points(origin, spacing, dims, real):
    """the nodes of a lattice as the interface defines them: (real)(origin + idx * spacing), formed in double; row (k * dy + j) * dx + i;
    (n, 4) with w = 1"""
    o = np.asarray(origin, np.float64)
    s = np.broadcast_to(np.asarray(spacing, np.float64), (3,))
    k, j, i = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    out = np.ones((i.size, 4), real)
    for a, idx in enumerate((i, j, k)):
        out[:, a] = (o[a] + idx.ravel().astype(np.float64) * s[a]).astype(real)
    return out


def _w(params, d, kernel_set, real):
    h = pm._p(params, "interactionRadius")
    if kernel_set == pm.MULLER:
        return pm.w_dens(d, h, pm._p(params, "kpoly"), real).astype(real)
    return pm.w_monaghan(d, h, real).astype(real)


def _gw(params, d, kernel_set, real):
    h = pm._p(params, "interactionRadius")
    if kernel_set == pm.MULLER:
        return pm.w_grad(d, h, pm._p(params, "kpoly_grad"), real).astype(real)
    return pm.w_monaghan_grad(d, h, real).astype(real)


def _sum(m, i, t):
    """(sum of t, sum of |t|) per query, in float64"""
    t = np.asarray(t, np.float64)
    return np.bincount(i, weights=t, minlength=m), np.bincount(i, weights=np.abs(t), minlength=m)


def sample(params, pos, vel, queries, kernel_set=pm.MULLER, bsorted=None):
    """The four fields at `queries` (m, >= 3) from the fluid (pos, vel) and, bsorted given, the wall term of the density.

    Returns a dict: count (m,) int; dens, dens_bound (m,); grad, grad_bound (m, 3); vel, vel_bound (m, 4) (w = the denominator);
    k (m,) the number of terms of the density sum (fluid + wall hits).  A query with a non-finite coordinate has no neighbour."""
    real = pm.real_of(params)
    eps = float(np.finfo(real).eps)
    h, m0, rd = pm._p(params, "interactionRadius"), pm._p(params, "particleMass"), pm._p(params, "restDensity")
    x = np.asarray(queries)[:, :3].astype(real)
    m = len(x)
    y = np.asarray(pos)[:, :3].astype(real)
    v = np.asarray(vel)[:, :3].astype(real)
    with np.errstate(invalid="ignore", over="ignore"):
        i, j = pm.pairs_within(x, y, h, real=real) if len(y) else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    fin = np.isfinite(x.astype(np.float64)).all(axis=1)
    keep = fin[i]
    i, j = i[keep], j[keep]
    d = x[i] - y[j]
    count = np.bincount(i, minlength=m)
    w = (real(m0) * _w(params, d, kernel_set, real)).astype(real)
    D, _ = _sum(m, i, w)
    dens, dens_a, k = D.copy(), D.copy(), count.copy()
    if bsorted is not None and len(bsorted):
        b = np.asarray(bsorted).astype(real)
        with np.errstate(invalid="ignore", over="ignore"):
            ib, jb = pm.pairs_within(x, b[:, :3], h, real=real)
        keep = fin[ib]
        ib, jb = ib[keep], jb[keep]
        db = x[ib] - b[jb, :3]
        psi = (real(rd) * b[jb, 3]).astype(real)
        sb, ab = _sum(m, ib, (psi * _w(params, db, kernel_set, real)).astype(real))
        dens, dens_a, k = dens + sb, dens_a + ab, k + np.bincount(ib, minlength=m)
    nz = pm._len(d) != 0
    g = (real(F32(m0)) * _gw(params, d[nz], kernel_set, real)).astype(real)
    grad, grad_a = np.zeros((m, 3)), np.zeros((m, 3))
    num, num_a = np.zeros((m, 3)), np.zeros((m, 3))
    t = (w.astype(F32).astype(real)[:, None] * v[j]).astype(real)
    for a in range(3):
        grad[:, a], grad_a[:, a] = _sum(m, i[nz], g[:, a])
        num[:, a], num_a[:, a] = _sum(m, i, t[:, a])
    kg = np.bincount(i[nz], minlength=m)
    out = dict(count=count, k=k, dens=dens, dens_bound=k * eps * dens_a, grad=grad, grad_bound=(kg * eps)[:, None] * grad_a)
    vel4, vb = np.zeros((m, 4)), np.zeros((m, 4))
    some = D > 0
    bD = count * eps * D
    bN = (count * eps)[:, None] * num_a
    with np.errstate(invalid="ignore", divide="ignore"):
        q = num / D[:, None]
        qb = (bN + np.abs(q) * bD[:, None]) / (D - bD)[:, None] * (1 + eps / 2) + (eps / 2) * np.abs(q)
    vel4[some, :3], vb[some, :3] = q[some], qb[some]
    vel4[some, 3], vb[some, 3] = D[some], bD[some]
    out.update(vel=vel4, vel_bound=vb)
    return out


def compare(got, want, what=""):
    """device results `got` ({field flag: array}) against sample()'s `want`: counts exact, exact zeros where the model has no term,
    everything else within the derived bound.  Prints and returns max(error / bound) per field."""
    ratios = {}
    if COUNT in got:
        np.testing.assert_array_equal(got[COUNT].astype(np.int64), want["count"], err_msg=what + " count")
    for flag, name, val, bound in ((DENSITY, "density", want["dens"], want["dens_bound"]), (GRADIENT, "gradient", want["grad"], want["grad_bound"]),
                                   (VELOCITY, "velocity", want["vel"], want["vel_bound"])):
        if flag not in got:
            continue
        g = np.asarray(got[flag], np.float64)
        if flag == GRADIENT:
            assert np.all(g[:, 3] == 0), what + " gradient w"
            g = g[:, :3]
        err = np.abs(g - val)
        zero = bound == 0
        assert np.all(err[zero] == 0), (what, name, "a value the model has no rounding for differs", float(err[zero].max()))
        r = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
        ratios[name] = r
        print("%s %s: max error / bound = %.3g" % (what, name, r))
        assert r <= 1.0, (what, name, r)
    return ratios
