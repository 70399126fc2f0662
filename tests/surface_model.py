"""Marching tetrahedra on the sampler's lattice, restated in numpy from the contract of include/nereus_hip.h "surface extraction"
(DESIGN.md "Surface extraction"), and checks of a mesh that need no model.

The model is vectorised over nodes and cells; the only Python loops run over the 7 edge directions, the 6 tetrahedra and the 14
non-empty cases of a tetrahedron.  It does not copy the device's case table: the edges of a case follow from the rule (one corner apart:
the edges from it to the others ascending; two and two: the quad ac, ad, bd, bc split along ac-bd), and the WINDING of every case from
geometry — the sign of the triangle's normal against the direction from the inside corners to the outside ones, with the vertices at the
edge midpoints of the unit cell.  (The sign does not depend on where the vertices sit on their edges: for one corner p apart, with e_i
the edge vectors from p and t_i the positions, n . (e1 + e2 + e3) = (t1 t2 + t2 t3 + t3 t1) det(e1, e2, e3); for the quad both normals
are multiples of (d - c) x (b - a) with positive factors.  So midpoints decide it also where a vertex has t = 0 and the real triangle is
degenerate.)

t and the vertex are formed in the build's real type with the contract's formula, one rounding per operation; the library is built
without contraction and with IEEE division, so the comparison with the device is exact: V, T, vertex and attribute bytes equal, the
triangles equal cell by cell as sets of cyclically normalised triples.
"""
import itertools

import numpy as np

EDGE_DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
PERMS = list(itertools.permutations(range(3)))  # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx
LOCAL_EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def tet_corners(perm):
    """the four corners of the Kuhn tetrahedron of a permutation (a, b, c), as (dx, dy, dz)"""
    a, b, _ = perm
    c1 = [0, 0, 0]
    c1[a] = 1
    c2 = list(c1)
    c2[b] = 1
    return [(0, 0, 0), tuple(c1), tuple(c2), (1, 1, 1)]


def case_triangles(perm, m):
    """the triangles of case m (bit c: local corner c inside) of a tetrahedron as triples of local edges (p, q), p < q, wound by geometry"""
    ins = [c for c in range(4) if (m >> c) & 1]
    outs = [c for c in range(4) if not (m >> c) & 1]
    if not ins or not outs:
        return []
    edge = lambda p, q: (min(p, q), max(p, q))
    if len(ins) == 1:
        tris = [[edge(ins[0], q) for q in outs]]
    elif len(outs) == 1:
        tris = [[edge(q, outs[0]) for q in ins]]
    else:
        (a, b), (c, d) = ins, outs
        ac, ad, bd, bc = edge(a, c), edge(a, d), edge(b, d), edge(b, c)
        tris = [[ac, ad, bd], [ac, bd, bc]]
    x = np.array(tet_corners(perm), np.float64)
    towards_outside = x[outs].mean(0) - x[ins].mean(0)
    wound = []
    for tri in tris:
        v = [(x[p] + x[q]) / 2 for p, q in tri]
        s = float(np.dot(np.cross(v[1] - v[0], v[2] - v[0]), towards_outside))
        assert s != 0.0
        wound.append(tri if s > 0 else [tri[0], tri[2], tri[1]])
    return wound


def lattice_axes(origin, spacing, dims, real):
    sp = np.broadcast_to(np.asarray(spacing, np.float64), (3,))
    return [(np.float64(origin[a]) + np.arange(dims[a], dtype=np.float64) * np.float64(sp[a])).astype(real) for a in range(3)]


def extract(dens, origin, spacing, dims, iso, real, attrs=None, tet_cases=False):
    """dens: (nodes,) in `real`, linear index (k * dims[1] + j) * dims[0] + i; attrs: {name: (nodes, 4) array} interpolated per vertex.
    Returns a dict: V, T, vertices (V, 4), triangles (T, 3) uint32, cell_counts (triangles of every cell, cells ascending), attrs; with
    tet_cases also tet_cases, a (6, 16) histogram: how many cells have Kuhn tetrahedron t (PERMS order) in sign case m (bit c: local
    corner c inside), taken from the inside mask alone."""
    nx, ny, nz = (int(d) for d in dims)
    f = np.ascontiguousarray(dens, dtype=real).reshape(nz, ny, nx)
    assert f.dtype == np.dtype(real)
    iso_r = np.dtype(real).type(iso)
    inside = f >= iso_r
    nodes = nx * ny * nz
    has = np.zeros((nodes, 7), bool)
    lin = np.arange(nodes).reshape(nz, ny, nx)
    far = np.zeros((nodes, 7), np.int64)
    for e, (dx, dy, dz) in enumerate(EDGE_DIRS):
        own = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        oth = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        has[lin[own].ravel(), e] = (inside[own] != inside[oth]).ravel()
        far[lin[own].ravel(), e] = lin[oth].ravel()
    vid = (np.cumsum(has.ravel()) - 1).reshape(nodes, 7)
    vid[~has] = -1
    node, e = np.nonzero(has)  # row-major: owner node ascending, then edge number ascending
    V = len(node)
    fl = f.ravel()
    f0, f1 = fl[node], fl[far[node, e]]
    t = (iso_r - f0) / (f1 - f0)
    ax = lattice_axes(origin, spacing, dims, real)
    idx = [node % nx, (node // nx) % ny, node // (nx * ny)]
    d = np.array(EDGE_DIRS)[e]
    vert = np.zeros((V, 4), real)
    for a in range(3):
        p0, p1 = ax[a][idx[a]], ax[a][np.minimum(idx[a] + d[:, a], dims[a] - 1)]
        vert[:, a] = p0 + t * (p1 - p0)
    vert[:, 3] = t
    out_attrs = {}
    for name, g in (attrs or {}).items():
        g = np.ascontiguousarray(g, dtype=real).reshape(nodes, 4)
        g0, g1 = g[node], g[far[node, e]]
        out_attrs[name] = g0 + t[:, None] * (g1 - g0)
    # triangles: cells ascending, then tet, then within the tet
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    ncell = cx * cy * cz
    tris = np.full((ncell, 6, 2, 3), -1, np.int64)
    vid3 = vid.reshape(nz, ny, nx, 7)
    hist = np.zeros((6, 16), np.int64)
    corner = lambda c: (slice(c[2], c[2] + cz), slice(c[1], c[1] + cy), slice(c[0], c[0] + cx))
    for ti, perm in enumerate(PERMS):
        cc = tet_corners(perm)
        m = np.zeros((cz, cy, cx), np.int64)
        for c in range(4):
            m |= inside[corner(cc[c])].astype(np.int64) << c
        m = m.ravel()
        hist[ti] = np.bincount(m, minlength=16)
        for case in range(1, 15):
            sel = np.nonzero(m == case)[0]
            if not len(sel):
                continue
            for s, tri in enumerate(case_triangles(perm, case)):
                for i, (p, q) in enumerate(tri):
                    en = EDGE_DIRS.index(tuple(np.subtract(cc[q], cc[p])))
                    ids = vid3[corner(cc[p])][..., en].ravel()[sel]
                    assert (ids >= 0).all()
                    tris[sel, ti, s, i] = ids
    counts = (tris[..., 0] >= 0).sum((1, 2))
    flat = tris.reshape(-1, 3)
    flat = flat[flat[:, 0] >= 0]
    out = {"V": V, "T": len(flat), "vertices": vert, "triangles": flat.astype(np.uint32), "cell_counts": counts, "attrs": out_attrs}
    if tet_cases:
        out["tet_cases"] = hist
    return out


def normalised(tri):
    """every triangle rotated so that its smallest index comes first (the winding is kept)"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    k = np.argmin(tri, axis=1)
    r = np.arange(len(tri))
    return np.stack([tri[r, k], tri[r, (k + 1) % 3], tri[r, (k + 2) % 3]], 1)


def compare(got_v, got_t, want, got_attrs=None, what=""):
    """bit-equality of a mesh (vertices (V, 4), triangles (T, 3)) with the model's; triangles as per-cell sets"""
    assert got_v.shape == want["vertices"].shape, (what, got_v.shape, want["vertices"].shape)
    assert got_t.shape == want["triangles"].shape, (what, got_t.shape, want["triangles"].shape)
    assert got_v.dtype == want["vertices"].dtype
    assert got_v.tobytes() == want["vertices"].tobytes(), (what, "vertex records differ", int((got_v != want["vertices"]).any(1).sum()))
    for name, a in (got_attrs or {}).items():
        w = want["attrs"][name]
        assert a.dtype == w.dtype and a.shape == w.shape and a.tobytes() == w.tobytes(), (what, "attribute %s differs" % name)
    # cell by cell: sort the normalised triples inside every cell's slice, then compare everything at once
    cell = np.repeat(np.arange(len(want["cell_counts"])), want["cell_counts"])
    keyed = []
    for tri in (got_t, want["triangles"]):
        n = normalised(tri)
        order = np.lexsort((n[:, 2], n[:, 1], n[:, 0], cell))
        keyed.append(n[order])
    assert np.array_equal(keyed[0], keyed[1]), (what, "triangles differ", int((keyed[0] != keyed[1]).any(1).sum()))


def mesh_checks(vertices, triangles, closed, lattice_volume=None):
    """Properties of an oriented mesh that need no model.  Every directed edge occurs at most once; every vertex is referenced; for a
    closed surface every directed edge's reverse occurs exactly once, V - E + F is even, and the signed volume sum x0 . (x1 x x2) / 6
    is > 0 and below the lattice's volume.  Returns (Euler characteristic or None, signed volume or None)."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    V = len(vertices)
    if len(tri) == 0:
        assert V == 0
        return None, None
    assert tri.min() >= 0 and tri.max() < V
    de = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    code = de[:, 0] * V + de[:, 1]
    assert len(np.unique(code)) == len(code), "a directed edge occurs twice"
    assert len(np.unique(tri)) == V, "a vertex is not referenced"
    if not closed:
        return None, None
    rev = de[:, 1] * V + de[:, 0]
    assert np.array_equal(np.sort(rev), np.sort(code)), "the surface is not closed"
    E = len(code) // 2
    chi = V - E + len(tri)
    assert chi % 2 == 0
    x = np.asarray(vertices, np.float64)[:, :3]
    x = x - x.mean(0)
    vol = float(np.einsum("ij,ij->i", x[tri[:, 0]], np.cross(x[tri[:, 1]], x[tri[:, 2]])).sum() / 6.0)
    assert vol > 0, vol
    if lattice_volume is not None:
        assert vol < lattice_volume, (vol, lattice_volume)
    return chi, vol
