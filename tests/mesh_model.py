"""numpy model of the mesh sampling (include/nereus_hip.h "mesh sampling"), written from the header's formulas: the field (generalised
winding number, squared distance, nearest triangle, closest point per lattice node) and the selection of nodes as particles.  Double
throughout; every product and sum is written out (no `@`, np.dot or einsum: BLAS may fuse or reorder), the triangles are walked in
ascending order and the nodes are the vectorised axis, so every IEEE-exact output has the bits the device computes.  Also the mesh
generators of the tests."""
import functools
import re
from pathlib import Path

import numpy as np

INSIDE, OUTSIDE, SNAP = 1, 2, 4
BATCH = 1 << 22   # MESH_BATCH of nrs_host_mesh.h
UNROLL = 4        # MESH_UNROLL of nrs_kernels_mesh.h (asserted equal in tests/test_mesh_model_cpu.py)
CSRC = Path(__file__).resolve().parents[1] / "nereus_amd" / "csrc"


def header_constant(header, name):
    """the integer value of `constexpr ... name = value;` in a csrc header (value may be written 1ull << k)"""
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, (CSRC / header).read_text())
    expr = re.sub(r"(\d+)(ull|u)\b", r"\1", m.group(1))
    return int(eval(expr, {"__builtins__": {}}))


# ---- the lattice ------------------------------------------------------------------------------------------------------------------------
def nodes(origin, spacing, dims, first=0, count=None):
    """(m, 3) double positions of the nodes first .. first+count-1 in linear index order (k * dims[1] + j) * dims[0] + i"""
    sp = np.broadcast_to(np.asarray(spacing, np.float64), (3,))
    total = int(dims[0]) * int(dims[1]) * int(dims[2])
    q = np.arange(first, total if count is None else first + count, dtype=np.int64)
    i = q % dims[0]
    t = q // dims[0]
    j = t % dims[1]
    k = t // dims[1]
    out = np.empty((len(q), 3), np.float64)
    for a, idx in enumerate((i, j, k)):
        out[:, a] = np.float64(origin[a]) + idx.astype(np.float64) * sp[a]
    return out


# ---- the field ----------------------------------------------------------------------------------------------------------------------------
def _sub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _along(o, d, s):
    return (o[0] + d[0] * s, o[1] + d[1] * s, o[2] + d[2] * s)


def _where3(c, u, v):
    return tuple(np.where(c, u[a], v[a]) for a in range(3))


def field(vertices, triangles, P, winding=True, distance=True):
    """the field at the points P (m, 3): dict with "winding", "dist2", "nearest", "closest" (those computed)"""
    V = np.asarray(vertices, np.float64).reshape(-1, 3)
    T = np.asarray(triangles, np.int64).reshape(-1, 3)
    P = np.asarray(P, np.float64)
    m = len(P)
    p = (P[:, 0].copy(), P[:, 1].copy(), P[:, 2].copy())
    acc = np.zeros(m)
    best = np.full(m, np.inf)
    bq = [np.zeros(m), np.zeros(m), np.zeros(m)]
    bt = np.full(m, 0xFFFFFFFF, np.uint32)
    ones = np.ones(m)
    with np.errstate(all="ignore"):
        for t in range(len(T)):
            A = tuple(V[T[t, 0], a] * ones for a in range(3))
            B = tuple(V[T[t, 1], a] * ones for a in range(3))
            Cc = tuple(V[T[t, 2], a] * ones for a in range(3))
            if winding:
                a, b, c = _sub(A, p), _sub(B, p), _sub(Cc, p)
                la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
                num = _dot(a, _cross(b, c))
                den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
                acc = acc + 2.0 * np.arctan2(num, den)
            if distance:
                ab, ac = _sub(B, A), _sub(Cc, A)
                ap, bp, cp = _sub(p, A), _sub(p, B), _sub(p, Cc)
                d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
                vc = d1 * d4 - d3 * d2
                vb = d5 * d2 - d1 * d6
                va = d3 * d6 - d5 * d4
                e43, e56 = d4 - d3, d5 - d6
                dn = 1.0 / (va + vb + vc)
                q = _along(_along(A, ab, vb * dn), ac, vc * dn)                                          # 7
                q = _where3((va <= 0.0) & (e43 >= 0.0) & (e56 >= 0.0), _along(B, _sub(Cc, B), e43 / (e43 + e56)), q)  # 6
                q = _where3((vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), _along(A, ac, d2 / (d2 - d6)), q)   # 5
                q = _where3((d6 >= 0.0) & (d5 <= d6), Cc, q)                                              # 4
                q = _where3((vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), _along(A, ab, d1 / (d1 - d3)), q)   # 3
                q = _where3((d3 >= 0.0) & (d4 <= d3), B, q)                                               # 2
                q = _where3((d1 <= 0.0) & (d2 <= 0.0), A, q)                                              # 1
                r = _sub(p, q)
                dd = _dot(r, r)
                win = dd < best
                best = np.where(win, dd, best)
                for a in range(3):
                    bq[a] = np.where(win, q[a], bq[a])
                bt = np.where(win, np.uint32(t), bt)
    out = {}
    if winding:
        out["winding"] = acc / (4.0 * np.pi)
    if distance:
        out["dist2"] = best
        out["nearest"] = bt.astype(np.uint32)
        out["closest"] = np.stack(bq, axis=1)
    return out


def lattice_field(vertices, triangles, origin, spacing, dims, **kw):
    return field(vertices, triangles, nodes(origin, spacing, dims), **kw)


# ---- the selection ------------------------------------------------------------------------------------------------------------------------
def selected(f, flags, dmin, dmax):
    """mask of the nodes of field f a rule selects"""
    both = (flags & (INSIDE | OUTSIDE)) == (INSIDE | OUTSIDE)
    if both:
        side = np.ones(len(f["dist2"]), bool)
    elif flags & INSIDE:
        side = f["winding"] > 0.5
    else:
        side = f["winding"] <= 0.5
    dmin2, dmax2 = np.float64(dmin) * np.float64(dmin), np.float64(dmax) * np.float64(dmax)
    return side & (dmin2 <= f["dist2"]) & (f["dist2"] <= dmax2)


def particles(f, P, flags, dmin, dmax, real):
    """(count, 4) particles of dtype real: the selected nodes P (or, with SNAP, their closest points), w = 1"""
    mask = selected(f, flags, dmin, dmax)
    src = f["closest"] if flags & SNAP else P
    out = np.ones((int(mask.sum()), 4), real)
    out[:, :3] = src[mask].astype(real)
    return out


# ---- meshes: (vertices (nv, 3) double, triangles (nt, 3) uint32), counter-clockwise seen from outside ------------------------------------------
def cube(lo, hi):
    """12 triangles; the two of the +z face come last"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (c >> a) & 1 else lo)[a] for a in range(3)] for c in range(8)], np.float64)
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]  # -x +x -y +y -z +z
    t = []
    for a, b, c, d in quads:
        t += [(a, b, c), (a, c, d)]
    return v, _outward(v, np.array(t, np.uint32), v.mean(axis=0))


def cup(lo, hi):
    """the cube without its +z face: 10 triangles, open"""
    v, t = cube(lo, hi)
    return v, t[:10].copy()


def _outward(v, t, centre):
    """flip the triangles whose normal points towards `centre` (star-shaped meshes)"""
    t = t.copy()
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    n = np.cross(b - a, c - a)
    flip = ((a + b + c) / 3.0 - centre)
    bad = (n * flip).sum(axis=1) < 0.0
    t[bad] = t[bad][:, [0, 2, 1]]
    return t


def icosphere(n, r=1.0, centre=(0.0, 0.0, 0.0)):
    """the icosahedron subdivided n times, vertices pushed to radius r: 20 * 4^n triangles"""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(x, np.float64) / np.sqrt(1.0 + g * g) for x in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(n):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.sqrt((x * x).sum()))
                mid[key] = len(v) - 1
            return mid[key]

        nt = []
        for a, b, c in t:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = nt
    c = np.asarray(centre, np.float64)
    vv = np.array(v) * np.float64(r) + c
    return vv, _outward(vv, np.array(t, np.uint32), c)


def torus(R, r, nu, nv, centre=(0.0, 0.0, 0.0)):
    """axis z, nu segments around the axis, nv around the tube: 2 * nu * nv triangles"""
    c = np.asarray(centre, np.float64)
    v = np.empty((nu * nv, 3), np.float64)
    for i in range(nu):
        u = 2.0 * np.pi * i / nu
        for j in range(nv):
            w = 2.0 * np.pi * j / nv
            v[i * nv + j] = ((R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w))
    v += c
    t = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            d, e = i * nv + (j + 1) % nv, ((i + 1) % nu) * nv + (j + 1) % nv
            t += [(a, b, e), (a, e, d)]
    return v, np.array(t, np.uint32)


# ---- the cases of the tests: name -> (vertices, triangles, origin, spacing, dims) -------------------------------------------------------------------
S = 0.02
CUBE_LO, CUBE_HI = (0.013, 0.007, 0.011), (0.213, 0.167, 0.191)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "cube":
        return cube(CUBE_LO, CUBE_HI) + ((-0.05, -0.05, -0.05), S, (16, 14, 15))
    if name == "icosphere":
        return icosphere(2, 0.11, (0.003, 0.001, 0.002)) + ((-0.15, -0.15, -0.15), S, (16, 16, 16))
    if name == "torus":
        return torus(0.12, 0.045, 16, 8, (0.001, 0.002, 0.003)) + ((-0.19, -0.19, -0.07), S, (20, 20, 8))
    if name == "cup":
        return cup(CUBE_LO, CUBE_HI) + ((-0.05, -0.05, -0.05), S, (16, 14, 15))
    raise KeyError(name)


CASES = ("cube", "icosphere", "torus", "cup")


@functools.lru_cache(maxsize=None)
def case_field(name):
    """the model's field on a case's lattice, computed once and shared (do not modify)"""
    v, t, o, s, d = case(name)
    f = lattice_field(v, t, o, s, d)
    for a in f.values():
        a.setflags(write=False)
    return f


def write_obj(path, vertices, faces):
    with open(path, "w") as fh:
        for x in np.asarray(vertices, np.float64):
            fh.write("v %.17g %.17g %.17g\n" % tuple(x))
        for f in faces:
            fh.write("f " + " ".join(str(int(i) + 1) for i in f) + "\n")
