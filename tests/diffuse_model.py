"""Numpy model of one nrs_diffuse_step (include/nereus_hip.h "diffuse particles"; DESIGN.md "Diffuse particles"), for the tests.

It restates nrs_host_diffuse.h and nrs_kernels_diffuse.h operation by operation in the build's precision `real` (SReal): every sum is
formed sequentially in `real`, in the device's order (the 27 cells of the owner's neighbourhood z, y, x ascending, sorted slots
ascending within a cell), every length is the device's float length() (pcisph_model._len), every product, quotient and difference is
rounded where the device rounds it (the library is built without contraction).  So the model is meant to agree with the device bit
for bit; the smoothing kernels are pcisph_model's through sample_model (pinned to the reference by test_model_kernels_pin.py).

Input is what the device reads: the downloaded fluid positions and velocities (the arrays the sampler's grid is built from) and the
living diffuse set of the previous step.  Neighbours are found by brute force.
"""
import numpy as np

from tests import pcisph_model as pm
from tests import sample_model as sm

F32 = np.float32
U64 = np.uint64
SPRAY, FOAM, BUBBLE = 0, 1, 2
DRAWS_PER_BIRTH = 10

DEFAULTS = dict(capacity=1 << 20, seed=0, tau_ta=(5.0, 20.0), tau_wc=(2.0, 8.0), tau_k=(5.0, 50.0), k_ta=4000.0, k_wc=50000.0,
                lifetime=(2.0, 5.0), k_buoyancy=2.0, k_drag=0.8, spray_below=6, bubble_above=20, max_per_particle=8)


def config(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


# ---- the uniform draws ----------------------------------------------------------------------------------------------------------------------
def _mix64(z):
    z = z ^ (z >> U64(30))
    z = z * U64(0xbf58476d1ce4e5b9)
    z = z ^ (z >> U64(27))
    z = z * U64(0x94d049bb133111eb)
    return z ^ (z >> U64(31))


def hash64(seed, step, slot, draw):
    """diffuse_hash: the splitmix64 finaliser on seed + golden * (step + 1), then on that xor (slot << 32 | draw); uint64 arrays"""
    with np.errstate(over="ignore"):
        seed, step = np.asarray(seed, U64), np.asarray(step, U64)
        a = _mix64(seed + U64(0x9e3779b97f4a7c15) * (step + U64(1)))
        w = (np.asarray(slot, U64) << U64(32)) | np.asarray(draw, U64)
        return _mix64(a ^ w)


def uniform(seed, step, slot, draw, real):
    """the top 24 bits times 2^-24"""
    return (hash64(seed, step, slot, draw) >> U64(40)).astype(real) * real(2.0 ** -24)


def birth_draw(k, t):
    return 1 + DRAWS_PER_BIRTH * np.asarray(k, np.int64) + t


def disc_point(ua, ub, real):
    """(a, b): the first of the four pairs (columns of ua, ub in [-1, 1]) inside the unit circle, else the centre"""
    a, b = np.zeros(len(ua), real), np.zeros(len(ua), real)
    done = np.zeros(len(ua), bool)
    for t in range(4):
        inside = (ua[:, t] * ua[:, t] + ub[:, t] * ub[:, t] < real(1)) & ~done
        a[inside], b[inside] = ua[inside, t], ub[inside, t]
        done |= inside
    return a, b


# ---- the grid: cells, the sampler's sorted order, neighbour pairs in the walk's order -----------------------------------------------------------
def _grid(params, real):
    wo = np.asarray(params["worldOrigin"]).reshape(-1)[:3].astype(real)
    cs = np.asarray(params["cellSize"]).reshape(-1)[:3].astype(real)
    gs = np.asarray(params["gridSize"]).reshape(-1)[:3].astype(np.int64)
    return wo, cs, gs


def cells(params, x, real):
    """calcGridPos: floor((p - worldOrigin) / cellSize), the quotient in `real`, converted to a 32-bit int the way the device converts
    (saturating; 0 for a NaN): the cell of a coordinate beyond +-2^31 cells or of a non-finite one is what the sampler's sort sees"""
    wo, cs, _ = _grid(params, real)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((np.asarray(x)[:, :3].astype(real) - wo) / cs).astype(np.float64)
    f = np.where(np.isnan(f), 0.0, np.clip(f, -2.0 ** 31, 2.0 ** 31 - 1))
    return f.astype(np.int64)


def dropped_pairs(params, owners, candidates, real, radius=None, reach=1, squared=False, same=False):
    """The number of pairs (owner i, candidate j) within `radius` (default h) whose cells lie more than `reach` apart on some axis: pairs
    that a model finding its pairs by distance alone counts and the device's walk over (2 reach + 1)^3 cells never meets.  The distance
    is the float length() of the difference in `real` (the sampler's test), or with squared the anisotropic pass's
    (dx dx + dy dy) + dz dz < radius^2 in `real`.  same: i != j.  The models that find pairs by brute force are the device's only on
    inputs where this is 0 (tests/test_readers_fuzz_cpu.py asserts it for every committed seed)."""
    r = real(pm._p(params, "interactionRadius") if radius is None else radius)
    x, y = np.asarray(owners)[:, :3].astype(real), np.asarray(candidates)[:, :3].astype(real)
    if not len(x) or not len(y):
        return 0
    cx, cy = cells(params, x, real), cells(params, y, real)
    rows = max(1, 2_000_000 // len(y))
    n = 0
    for a in range(0, len(x), rows):
        with np.errstate(invalid="ignore", over="ignore"):
            d = x[a:a + rows, None, :] - y[None, :, :]
            if squared:
                near = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] < r * r
            else:
                near = pm._len(d).astype(np.float64) < float(r)
        i, j = np.nonzero(near)
        i = i + a
        far = (np.abs(cy[j] - cx[i]) > reach).any(axis=1)
        if same:
            far &= i != j
        n += int(far.sum())
    return n


def sorted_order(params, pos, real):
    """the sampler's sorted order: cell hash ascending, ties by array index (a stable radix sort of (hash, index))"""
    _, _, gs = _grid(params, real)
    c = cells(params, pos, real) & (gs - 1)
    h = (c[:, 2] * gs[1] + c[:, 1]) * gs[0] + c[:, 0]
    return np.argsort(h, kind="stable")


def walk_pairs(params, x, y, real, same=False):
    """(i, j, d) with length(x_i - y_j) < h and y_j in one of the 27 cells around x_i's, in the order the walk meets them: i ascending,
    then the cell offset z, y, x ascending, then j ascending; d = x_i - y_j in `real`; same: j != i"""
    h = float(real(pm._p(params, "interactionRadius")))
    x, y = np.asarray(x)[:, :3].astype(real), np.asarray(y)[:, :3].astype(real)
    if not len(x) or not len(y):
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3), real)
    cx, cy = cells(params, x, real), cells(params, y, real)
    rows = max(1, 2_000_000 // len(y))
    out = []
    for a in range(0, len(x), rows):
        with np.errstate(invalid="ignore", over="ignore"):
            ln = pm._len(x[a:a + rows, None, :] - y[None, :, :]).astype(np.float64)
        i, j = np.nonzero(ln < h)
        i = i + a
        off = cy[j] - cx[i]
        keep = (np.abs(off) <= 1).all(axis=1)
        if same:
            keep &= i != j
        i, j, off = i[keep], j[keep], off[keep]
        key = ((off[:, 2] + 1) * 3 + (off[:, 1] + 1)) * 3 + (off[:, 0] + 1)
        o = np.lexsort((j, key, i))
        out.append((i[o], j[o]))
    i, j = np.concatenate([p[0] for p in out]), np.concatenate([p[1] for p in out])
    return i, j, x[i] - y[j]


def seq_sum(m, i, t, real):
    """per owner the sum of its terms t in the order given (i ascending), one accumulator in `real`"""
    acc = np.zeros(m, real)
    if not len(i):
        return acc
    t = np.asarray(t, real)
    cnt = np.bincount(i, minlength=m)
    start = np.concatenate(([0], np.cumsum(cnt)[:-1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(int(cnt.max())):
            sel = np.nonzero(cnt > r)[0]
            acc[sel] = acc[sel] + t[start[sel] + r]
    return acc


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), axis=1)


def _unit_neg(g, real):
    """-g / length(g) per row; zero rows (and ok False) where the length is 0"""
    gl = pm._len(g)
    ok = gl != 0
    n = np.zeros_like(g)
    with np.errstate(invalid="ignore", divide="ignore"):
        n[ok] = (-g[ok]) / gl[ok].astype(real)[:, None]
    return n, ok


def _clamp(x, lo, hi, real):
    lo, hi = real(lo), real(hi)
    return (np.where(x < hi, x, hi) - np.where(x < lo, x, lo)) / (hi - lo)


def kind_of(n, cfg):
    n = np.asarray(n)
    return np.where(n < cfg["spray_below"], SPRAY, np.where(n > cfg["bubble_above"], BUBBLE, FOAM)).astype(np.uint32)


# ---- the passes of a step ---------------------------------------------------------------------------------------------------------------------
def fluid_pass(params, cfg, pos, vel, step, dt, kernel_set=pm.MULLER, raw=False):
    """normals, potentials and births per SORTED fluid particle; dict with order, spos, svel, normals (N, 3), potentials (N, 4), births,
    parent_kind; raw: also the unclamped potentials (ta, wc, ek)"""
    real = pm.real_of(params)
    order = sorted_order(params, pos, real)
    sx, sv = np.asarray(pos)[order, :3].astype(real), np.asarray(vel)[order, :3].astype(real)
    n = len(sx)
    h, m0 = real(pm._p(params, "interactionRadius")), real(pm._p(params, "particleMass"))
    i, j, d = walk_pairs(params, sx, sx, real, same=True)
    ln = pm._len(d)
    nz = ln != 0
    # 1. the density gradient: the sampler's gradient term at the particles
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = real(F32(m0)) * sm._gw(params, d[nz], kernel_set, real)
    grad = np.stack([seq_sum(n, i[nz], g[:, a], real) for a in range(3)], axis=1) if n else np.zeros((0, 3), real)
    # 2. the potentials
    nhat, nok = _unit_neg(grad, real)
    vl_i = pm._len(sv)
    with np.errstate(invalid="ignore", divide="ignore"):
        gate = nok & (vl_i != 0) & (_dot(sv, nhat) / vl_i.astype(real) >= real(0.6))
        r = ln.astype(real)
        wl = real(1) - r / h
        vij = sv[i] - sv[j]
        vl = pm._len(vij)
        lv = vl.astype(real)
        cs = _dot(vij, d) / (lv * r)
        om = real(1) - cs
        t_ta = lv * np.where(om > 0, om, real(0)) * wl   # (float lengths in an fp64 build: the cosine may pass 1 by a float ulp)
        ok_ta = nz & (vl != 0)
        om = real(1) - _dot(nhat[i], nhat[j])
        t_wc = np.where(om > 0, om, real(0)) * wl
        ok_wc = nz & gate[i] & (_dot(d, nhat[i]) > 0) & nok[j]
    ta = seq_sum(n, i[ok_ta], t_ta[ok_ta], real)
    wc = seq_sum(n, i[ok_wc], t_wc[ok_wc], real)
    ek = (real(0.5) * m0) * _dot(sv, sv)
    ita, iwc, ik = _clamp(ta, *cfg["tau_ta"], real), _clamp(wc, *cfg["tau_wc"], real), _clamp(ek, *cfg["tau_k"], real)
    rate = ik * (real(cfg["k_ta"]) * ita + real(cfg["k_wc"]) * iwc)
    u = uniform(cfg["seed"], step, np.arange(n), 0, real)
    births = births_count(cfg, rate, dt, u, real)
    cnt = 1 + np.bincount(i, minlength=n)
    out = dict(order=order, spos=sx, svel=sv, normals=grad, potentials=np.stack((ita, iwc, ik, rate), axis=1).astype(real), births=births,
               parent_kind=kind_of(cnt, cfg), count=cnt)
    if raw:
        out.update(ta=ta, wc=wc, ek=ek, gate=gate)
    return out


def shepard(params, sx, sv, x, kernel_set=pm.MULLER):
    """sample_walk at the positions x over the sorted fluid: (Shepard velocity (m, 3), 0 where nothing is near; neighbour count)"""
    real = pm.real_of(params)
    m0 = real(pm._p(params, "particleMass"))
    m = len(x)
    i, j, d = walk_pairs(params, x, sx, real)
    w = (m0 * sm._w(params, d, kernel_set, real)).astype(real)
    wf = w.astype(F32).astype(real)   # (the float scalar of scalar * vector)
    wsum = seq_sum(m, i, w, real)
    vt = np.zeros((m, 3), real)
    some = wsum != 0
    for a in range(3):
        num = seq_sum(m, i, wf * sv[j, a], real)
        with np.errstate(invalid="ignore", divide="ignore"):
            vt[some, a] = num[some] / wsum[some]
    return vt, np.bincount(i, minlength=m)


def advect_rule(cfg, x, v, life, vt, n, g, dt, lo, hi, real):
    """diffuse_advect on arrays: (new x, new v, new life, kind, alive) from positions x, velocities v, lifetimes, the Shepard velocities
    vt and neighbour counts n; g gravity, [lo, hi) the grid box"""
    dt = real(dt)
    x, v, vt, life = np.asarray(x, real), np.asarray(v, real), np.asarray(vt, real), np.asarray(life, real)
    g, lo, hi = np.asarray(g, real), np.asarray(lo, real), np.asarray(hi, real)
    kind = kind_of(n, cfg)
    spray, foam = (kind == SPRAY)[:, None], (kind == FOAM)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        v_s = v + dt * g
        nb = -real(cfg["k_buoyancy"])
        v_b = (v + dt * (nb * g)) + real(cfg["k_drag"]) * (vt - v)
        vn = np.where(spray, v_s, np.where(foam, vt, v_b)).astype(real)
        life = np.where(kind == FOAM, life - dt, life).astype(real)
        xn = x + dt * vn
        alive = (life > 0) & ((xn >= lo) & (xn < hi)).all(axis=1)
    return xn, vn, life, kind, alive


def advect(params, cfg, sx, sv, dpos, dvel, dt, kernel_set=pm.MULLER):
    """the living set one step on: (pos4, vel4, kind, alive mask), all of the input's length (dead rows hold what they moved to)"""
    real = pm.real_of(params)
    p4, v4 = np.asarray(dpos, real).reshape(-1, 4), np.asarray(dvel, real).reshape(-1, 4)
    x, v, life = p4[:, :3].copy(), v4[:, :3].copy(), p4[:, 3].copy()
    fin = np.isfinite(x).all(axis=1)
    xq = np.where(fin[:, None], x, real(0))
    vt, n = shepard(params, sx, sv, xq, kernel_set) if len(sx) else (np.zeros_like(x), np.zeros(len(x), np.int64))
    g = np.asarray(params["gravity"]).reshape(-1)[:3].astype(real)
    wo, cs, gs = _grid(params, real)
    hi = wo + gs.astype(real) * cs
    xn, vn, life, kind, alive = advect_rule(cfg, x, v, life, vt, n, g, dt, wo, hi, real)
    alive &= fin
    return np.concatenate((xn, life[:, None]), axis=1), np.concatenate((vn, np.zeros((len(vn), 1), real)), axis=1), kind, alive


def birth_rule(cfg, step, slot, k, xi, vi, rv, dt, real):
    """diffuse_birth on arrays: (x, v, lifetime) of birth k of the fluid particle (xi, vi) of sorted slot `slot`"""
    dt, rv = real(dt), real(rv)
    xi, vi = np.asarray(xi, real).reshape(-1, 3), np.asarray(vi, real).reshape(-1, 3)
    slot, k = np.asarray(slot, np.int64), np.asarray(k, np.int64)
    seed = cfg["seed"]
    one, two = real(1), real(2)
    ua = np.stack([two * uniform(seed, step, slot, birth_draw(k, 2 * t), real) - one for t in range(4)], axis=1).reshape(-1, 4)
    ub = np.stack([two * uniform(seed, step, slot, birth_draw(k, 2 * t + 1), real) - one for t in range(4)], axis=1).reshape(-1, 4)
    a, bb = disc_point(ua, ub, real)
    xh, xl = uniform(seed, step, slot, birth_draw(k, 8), real), uniform(seed, step, slot, birth_draw(k, 9), real)
    e1, e2 = frame(vi, real)
    ra, rb, s = (rv * a)[:, None], (rv * bb)[:, None], (xh * dt)[:, None]
    off = ra * e1 + rb * e2
    x = (xi + off) + s * vi
    v = vi + off
    lmin, lmax = real(cfg["lifetime"][0]), real(cfg["lifetime"][1])
    return x.astype(real), v.astype(real), (lmin + xl * (lmax - lmin)).astype(real)


def births_of(params, cfg, F, step, dt):
    """the births of a fluid pass in their order (slot, then birth number): (pos4, vel4, kind)"""
    real = pm.real_of(params)
    b = F["births"].astype(np.int64)
    slot = np.repeat(np.arange(len(b)), b)
    k = np.arange(len(slot)) - np.repeat(np.cumsum(b) - b, b)
    x, v, life = birth_rule(cfg, step, slot, k, F["spos"][slot], F["svel"][slot], pm._p(params, "particleRadius"), dt, real)
    return np.concatenate((x, life[:, None]), axis=1), np.concatenate((v, np.zeros((len(v), 1), real)), axis=1), F["parent_kind"][slot]


def births_count(cfg, rate, dt, u, real):
    """diffuse_births: min(floor(rate dt + u), max_per_particle); 0 for a NaN"""
    mp = cfg["max_per_particle"]
    with np.errstate(invalid="ignore"):
        t = np.asarray(rate, real) * real(dt) + np.asarray(u, real)
        return np.where(t >= real(mp), mp, np.where(t > 0, np.floor(t), 0)).astype(np.uint32)


def frame(v, real):
    """(e1, e2) of diffuse_birth: vhat = v / length(v); e1 = normalised vhat x axis, axis the coordinate axis of vhat's smallest absolute
    component (the lowest on a tie); e2 = vhat x e1; (x, y) where length(v) is 0"""
    v = np.asarray(v, real).reshape(-1, 3)
    m = len(v)
    e1, e2 = np.zeros((m, 3), real), np.zeros((m, 3), real)
    e1[:, 0], e2[:, 1] = 1, 1
    vl = pm._len(v) if m else np.zeros(0, F32)
    ok = vl != 0
    if ok.any():
        vh = v[ok] / vl[ok].astype(real)[:, None]
        ab = np.abs(vh)
        ax = np.where((ab[:, 0] <= ab[:, 1]) & (ab[:, 0] <= ab[:, 2]), 0, np.where(ab[:, 1] <= ab[:, 2], 1, 2))
        axis = np.zeros_like(vh)
        axis[np.arange(len(vh)), ax] = 1
        t1 = _cross(vh, axis)
        f1 = t1 / pm._len(t1).astype(real)[:, None]
        e1[ok], e2[ok] = f1, _cross(vh, f1)
    return e1, e2


def step(params, cfg, fpos, fvel, dpos, dvel, step_index, dt=0.0, kernel_set=pm.MULLER, capacity=None, raw=False):
    """One nrs_diffuse_step.  fpos / fvel: the downloaded fluid; dpos / dvel: the living set before ((D, 4) each, pos.w = lifetime);
    step_index: diffuse steps since configure; dt 0: the parameters' timestep; capacity None: cfg's.  Returns a dict: pos, vel, kind (the
    living set after), alive, by_kind, dropped (of this step), survivors, total (survivors + births before the capacity), and the fluid
    pass (normals (N, 4), potentials, births, F)."""
    real = pm.real_of(params)
    dt = real(dt) if dt else real(pm._p(params, "timestep"))
    cap = cfg["capacity"] if capacity is None else capacity
    F = fluid_pass(params, cfg, fpos, fvel, step_index, dt, kernel_set, raw=raw)
    p4, v4, kind, alive = advect(params, cfg, F["spos"], F["svel"], dpos, dvel, dt, kernel_set)
    bp, bv, bk = births_of(params, cfg, F, step_index, dt)
    pos, vel, kinds = np.concatenate((p4[alive], bp)), np.concatenate((v4[alive], bv)), np.concatenate((kind[alive], bk))
    total = len(pos)
    keep = min(total, cap)
    n = len(F["spos"])
    return dict(pos=pos[:keep], vel=vel[:keep], kind=kinds[:keep].astype(np.uint32), alive=keep, dropped=total - keep, survivors=int(alive.sum()),
                total=total, by_kind=[int((kinds[:keep] == k).sum()) for k in range(3)],
                normals=np.concatenate((F["normals"], np.zeros((n, 1), real)), axis=1), potentials=F["potentials"], births=F["births"], F=F)
