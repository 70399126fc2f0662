"""Numpy model of the anisotropic surface reconstruction (include/nereus_hip.h "anisotropic surface reconstruction"; DESIGN.md
"Anisotropic kernels"; Yu & Turk 2013), for the tests.

records(): pass A by brute force.  The MEMBERSHIP of a neighbourhood is formed exactly as the contract writes it, in the build's real
type R: d = x_j - x_i per component, d2 = (dx dx + dy dy) + dz dz, neighbour when d2 < r2 with r = (R)2 h, r2 = r r — so counts are
exact.  Everything after that is float64: the weights, the five sums, the centre, the covariance, numpy.linalg.eigh for the axes, the
clamps and G.  The device differs by the rounding of its sums and of its eigen solve in R only.

field(): pass B by brute force FROM GIVEN RECORDS (the device's own, as downloaded), in float64, with an a-priori bound on what the
device's evaluation in R may differ by.  With eps the machine epsilon of R (twice the unit roundoff, which pays for the second-order
terms left out), per candidate:

    d_k   = x_k - c_k                  one rounding                        |err| <= eps |d_k|
    g_i   = sum_k G_ik d_k             3 products, 2 sums, the error of d  |err| <= 4 eps ga_i,           ga_i = sum_k |G_ik| |d_k|
    q2    = sum_i g_i^2                                                    |err| <= eq = 8 eps sum_i |g_i| ga_i + 3 eps q2
    p     = 1 - q2                                                         |err| <= ep = eq + eps p
    t     = (w (p p)) p                3 roundings                         |err| <= et = w ((p + ep)^3 - p^3) + 3 eps t
    h_c   = sum_k G_ck g_k                                                 |err| <= eh_c = 4 eps sum_k |G_ck| ga_k + 3 eps sum_k |G_ck| |g_k|
    grad_c term = (-6 (w (p p))) h_c                                       |err| <= 6 w (((p + ep)^2 - p^2)(|h_c| + eh_c) + p^2 eh_c) + 4 eps |term|
    vel_c term  = t v_c                                                    |err| <= et |v_c| + eps |t v_c|

A candidate the two sides may decide differently is covered: one the model keeps and the device drops at q2 < 1 has p <= ep, and
p^3 <= (p + ep)^3 - p^3; one the model drops (q2 in [1, 1 + eq): p is taken as 0) and the device keeps has t <= w ep^3, which is et at
p = 0.  The first test, d2 < bound^2, is decided in R from three products and two sums: a candidate with d2 within 4 eps of bound^2
is kept by the model, and its whole |term| is added to the bound.  The sum of k kept terms adds k eps sum |term| (sample_model.py has
that derivation), so

    |phi_device - phi| <= k eps sum |t| + sum et,        the same for each gradient component,

and the velocity is the quotient of two such sums plus the rounding of the division, bounded as in sample_model.py.  A node without a
candidate is exactly 0 on both sides.
"""
import numpy as np

F32 = np.float32
DEFAULTS = dict(support=None, lam=0.9, k_r=4.0, k_n=0.5, n_eps=25)
K315 = 315.0 / (64.0 * np.pi)


def config(h, **kw):
    c = dict(DEFAULTS)
    c.update(kw)
    if not c["support"]:
        c["support"] = h
    return c


def neighbours(pos, h, real):
    """(N, N) bool: j is a neighbour of i, decided in `real` exactly as the contract writes it; and d = x_j - x_i in `real` (N, N, 3)"""
    x = np.asarray(pos)[:, :3].astype(real)
    r = real(2) * real(h)
    r2 = r * r
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[None, :, :] - x[:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        nb = d2 < r2
    fin = np.isfinite(x.astype(np.float64)).all(axis=1)
    nb &= fin[:, None]
    return nb, d, float(r)


def axes_of(sig, count, cfg, h):
    """semi-axes (N, 3) for eigenvalues sig (N, 3), any order"""
    s1 = sig.max(axis=1)
    a = np.full(sig.shape, cfg["k_n"] * cfg["support"])
    an = (count >= cfg["n_eps"]) & (s1 > 0)
    st = np.maximum(sig[an], (s1[an] / cfg["k_r"])[:, None])
    a[an] = cfg["support"] * st / np.cbrt(st.prod(axis=1))[:, None]
    return np.minimum(a, 1.5 * h)


def finish(sw, M, S, D, count, x, h, r, cfg):
    """the finishing routine in float64: sums (sw (N,), M (N, 3), S (N, 3, 3), D (N,), count) -> the records"""
    n = len(sw)
    out = dict(center=np.array(x, np.float64), bound=np.zeros(n), G=np.zeros((n, 3, 3)), weight=np.zeros(n), count=count, axes=np.zeros((n, 3)))
    ok = (count > 0) & (sw > 0) & (D > 0)
    if not ok.any():
        return out
    mu = M[ok] / sw[ok, None]
    delta = cfg["lam"] * mu
    dl = np.linalg.norm(delta, axis=1)
    lng = dl > 0.5 * h
    delta[lng] *= (0.5 * h / dl[lng])[:, None]
    out["center"][ok] = np.asarray(x, np.float64)[ok] + delta
    C = S[ok] / sw[ok, None, None] - mu[:, :, None] * mu[:, None, :]
    sig, U = np.linalg.eigh(C)
    a = axes_of(sig, count[ok], cfg, h)
    out["axes"][ok] = a
    out["U"] = U
    out["G"][ok] = np.einsum("nik,nk,njk->nij", U, 1.0 / a, U)
    k6 = 315.0 / (64.0 * np.pi * r ** 9)
    out["weight"][ok] = K315 / (k6 * D[ok]) / a.prod(axis=1)
    out["bound"][ok] = a.max(axis=1)
    return out


def records(pos, h, real, **kw):
    """pass A on positions (N, >= 3), in input order: dict of center (N, 3), bound, G (N, 3, 3), weight, count, axes (N, 3)"""
    cfg = config(h, **kw)
    nb, d, r = neighbours(pos, h, real)
    d = np.where(nb[..., None], d.astype(np.float64), 0.0)
    dl = np.sqrt((d * d).sum(-1))
    w = np.where(nb, 1.0 - (dl / r) ** 3, 0.0)
    sw = w.sum(1)
    M = np.einsum("ij,ijk->ik", w, d)
    S = np.einsum("ij,ijk,ijl->ikl", w, d, d)
    D = np.where(nb, (r * r - dl * dl) ** 3, 0.0).sum(1)
    x = np.asarray(pos)[:, :3].astype(real).astype(np.float64)
    return finish(sw, M, S, D, nb.sum(1), x, h, r, cfg)


def unpack(center4, g8):
    """the device's records as float64: centre (N, 3), bound (N,), G (N, 3, 3), weight (N,)"""
    c = np.asarray(center4, np.float64)
    g = np.asarray(g8, np.float64).reshape(-1, 8)
    G = np.empty((len(c), 3, 3))
    G[:, 0, 0], G[:, 0, 1], G[:, 0, 2], G[:, 1, 1], G[:, 1, 2], G[:, 2, 2] = g[:, 0], g[:, 1], g[:, 2], g[:, 3], g[:, 4], g[:, 5]
    G[:, 1, 0], G[:, 2, 0], G[:, 2, 1] = G[:, 0, 1], G[:, 0, 2], G[:, 1, 2]
    assert not g[:, 7].any()
    return c[:, :3], c[:, 3], G, g[:, 6]


def field(center, bound, G, weight, vel, queries, real, chunk=4096):
    """pass B at `queries` (m, >= 3; already in `real`) from records in float64; vel (N, 3) or None.  Returns a dict: phi, phi_bound (m,);
    grad, grad_bound (m, 3); vel, vel_bound (m, 4) (w = phi); k (m,) kept candidates"""
    eps = float(np.finfo(real).eps)
    x = np.asarray(queries)[:, :3].astype(np.float64)
    m = len(x)
    fin = np.isfinite(x).all(axis=1)
    use = np.isfinite(center).all(axis=1) & (bound > 0)
    cu, bu, Gu, wu = center[use], bound[use], G[use], weight[use]
    vu = np.asarray(vel, np.float64)[use, :3] if vel is not None else np.zeros((int(use.sum()), 3))
    phi, phib, k = np.zeros(m), np.zeros(m), np.zeros(m, np.int64)
    grad, gradb, num, numb, numa = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 3))
    phia, grada = np.zeros(m), np.zeros((m, 3))
    b2 = bu * bu
    for s in range(0, m, chunk):
        xs = np.where(fin[s:s + chunk, None], x[s:s + chunk], np.inf)
        with np.errstate(invalid="ignore"):
            d2 = ((xs[:, None, :] - cu[None, :, :]) ** 2).sum(-1)
        qi, j = np.nonzero(d2 < b2[None, :] * (1 + 4 * eps))
        band = d2[qi, j] >= b2[j] * (1 - 4 * eps)
        d = xs[qi] - cu[j]
        Gj, Ga = Gu[j], np.abs(Gu[j])
        g = np.einsum("nik,nk->ni", Gj, d)
        ga = np.einsum("nik,nk->ni", Ga, np.abs(d))
        q2 = (g * g).sum(1)
        eq = 8 * eps * (np.abs(g) * ga).sum(1) + 3 * eps * q2
        keep = q2 < 1 + eq
        qi, j, band, g, ga, q2, eq, Gj, Ga = qi[keep], j[keep], band[keep], g[keep], ga[keep], q2[keep], eq[keep], Gj[keep], Ga[keep]
        p = np.maximum(1 - q2, 0.0)
        ep = eq + eps * p
        w = wu[j]
        t = w * p ** 3
        et = w * ((p + ep) ** 3 - p ** 3) + 3 * eps * t + np.where(band, t, 0.0)
        hh = np.einsum("nik,nk->ni", Gj, g)
        eh = 4 * eps * np.einsum("nik,nk->ni", Ga, ga) + 3 * eps * np.einsum("nik,nk->ni", Ga, np.abs(g))
        gt = (-6 * w * p * p)[:, None] * hh
        egt = (6 * w)[:, None] * ((((p + ep) ** 2 - p * p))[:, None] * (np.abs(hh) + eh) + (p * p)[:, None] * eh) + 4 * eps * np.abs(gt) + np.where(band[:, None], np.abs(gt), 0.0)
        vt = t[:, None] * vu[j]
        evt = et[:, None] * np.abs(vu[j]) + eps * np.abs(vt)
        qq = qi + s
        k += np.bincount(qq, minlength=m)
        phi += np.bincount(qq, weights=t, minlength=m)
        phia += np.bincount(qq, weights=np.abs(t), minlength=m)
        phib += np.bincount(qq, weights=et, minlength=m)
        for a in range(3):
            grad[:, a] += np.bincount(qq, weights=gt[:, a], minlength=m)
            grada[:, a] += np.bincount(qq, weights=np.abs(gt[:, a]), minlength=m)
            gradb[:, a] += np.bincount(qq, weights=egt[:, a], minlength=m)
            num[:, a] += np.bincount(qq, weights=vt[:, a], minlength=m)
            numa[:, a] += np.bincount(qq, weights=np.abs(vt[:, a]), minlength=m)
            numb[:, a] += np.bincount(qq, weights=evt[:, a], minlength=m)
    phib += k * eps * phia
    gradb += (k * eps)[:, None] * grada
    bN = numb + (k * eps)[:, None] * numa
    vel4, vb = np.zeros((m, 4)), np.zeros((m, 4))
    some = phi > phib
    with np.errstate(invalid="ignore", divide="ignore"):
        q = num / phi[:, None]
        qb = (bN + np.abs(q) * phib[:, None]) / (phi - phib)[:, None] * (1 + eps / 2) + (eps / 2) * np.abs(q)
    vel4[some, :3], vb[some, :3] = q[some], qb[some]
    vel4[some, 3], vb[some, 3] = phi[some], phib[some]
    return dict(phi=phi, phi_bound=phib, grad=grad, grad_bound=gradb, vel=vel4, vel_bound=vb, vel_checked=some, k=k)


def poly6_density(pos, queries, h, kpoly, mass, chunk=4096):
    """the raw SPH density sum_j m kpoly (h^2 - r^2)^3 at the queries, float64 (the field nrs_surface_extract meshes, Mueller kernels)"""
    x = np.asarray(queries)[:, :3].astype(np.float64)
    y = np.asarray(pos)[:, :3].astype(np.float64)
    out = np.zeros(len(x))
    for s in range(0, len(x), chunk):
        d2 = ((x[s:s + chunk, None, :] - y[None, :, :]) ** 2).sum(-1)
        out[s:s + chunk] = (mass * kpoly * np.where(d2 < h * h, h * h - d2, 0.0) ** 3).sum(1)
    return out


def components(triangles, nverts):
    """connected components of a mesh's vertices (union-find over its edges)"""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    parent = np.arange(nverts)
    a = np.concatenate([tri[:, 0], tri[:, 1]])
    b = np.concatenate([tri[:, 1], tri[:, 2]])
    while True:
        pa, pb = parent[a], parent[b]
        lo = np.minimum(pa, pb)
        before = parent.copy()
        np.minimum.at(parent, pa, lo)
        np.minimum.at(parent, pb, lo)
        parent = parent[parent]
        if np.array_equal(parent, before):
            break
    return len(np.unique(parent))


def padded_lattice(pos, h, spacing, pad=2.5):
    """(origin, dims) of the lattice at `spacing` over the particles' bounding box inflated by pad * h (>= 2: a border node is farther
    than h / 2 + 3 h / 2 from every particle, no ellipsoid reaches it)"""
    p = np.asarray(pos)[:, :3].astype(np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    lo, hi = p.min(0) - pad * h, p.max(0) + pad * h
    return tuple(float(v) for v in lo), tuple(int(np.ceil((hi[a] - lo[a]) / spacing)) + 1 for a in range(3))
