"""A numpy model of WHICH waves of the LDS-staged density launch (nrs_kernels_staged.h, NRS_FLAG_STAGED_SCAN) stage their neighbour
rows, and of the hit counts the launch publishes — written from the kernel's stated rules, not from its code path by path:

  * one wave owns 64 consecutive sorted slots;
  * a wave with an active lane in a grid-edge cell (cell coordinate 0 or gridSize - 1 on any axis) takes the global-memory scan;
  * per lane and per (dz, dy) row the run [lo, hi) of the sorted array is the x-1 .. x+1 cells of that row (first non-empty cell's
    start to last non-empty cell's end; an empty row is lo = hi); the row's hull over the wave is [lo of the first lane with a
    non-empty run, hi of the last];
  * a wave stages iff, for every z-plane, its three hull lengths sum to at most STG_POOL = 320;
  * a fluid candidate is a hit when the float dot product of the float difference is below lenLtIr, a boundary candidate (lists
    shared with the force kernel, Muller) when it is below r2LeH2 — the two cut-offs of make_thresholds (nrs_host_scan.h);
  * a list overflows when nf + nb > HIT_CAP = 20, and an owner with a non-finite coordinate counts as overflowed.

Inputs are the sorted state of the step (sorted positions, sorted cell keys, the cell tables, the boundary tables and sorted boundary
positions) as the CPU oracle leaves it; nothing here comes from the device.  Grids: powers of two, every axis >= 4 cells (the 27
cells of a particle are then distinct), single domain."""
import numpy as np

WAVE = 64
POOL = 320        # STG_POOL: float4 slots per wave and z-plane
HIT_CAP = 20
COOP_LANES = 4    # STG_COOP_LANES: up to this many lanes with boundary cells are swept by the whole wave
EMPTY = 0xFFFFFFFF


def make_thresholds(ir):
    """CutThresholds for SReal = float, by the definition in nrs_host_scan.h:
    lenLtIr: the smallest float T with sqrtf(T) >= ir; r2LeH2: the smallest float T with fl(sqrtf(T)^2) > fl(ir * ir)."""
    f = np.float32
    ir = f(ir)
    up, down = f(np.inf), f(0.0)

    def search(pred):
        t = f(ir * ir)
        while pred(t) and t > 0:
            t = np.nextafter(t, down)
        while not pred(t):
            t = np.nextafter(t, up)
        return f(t)

    h2 = f(ir * ir)
    len_lt_ir = search(lambda x: not (np.sqrt(f(x)) < ir))
    r2_le_h2 = search(lambda x: f(np.sqrt(f(x)) * np.sqrt(f(x))) > h2)
    return len_lt_ir, r2_le_h2


def _grid(params):
    gs = np.asarray(params["gridSize"]).reshape(-1)[:3].astype(np.int64)
    assert np.all(gs >= 4) and np.all(gs & (gs - 1) == 0), gs
    return gs


def _cells(hash_, gs):
    h = np.asarray(hash_).astype(np.int64)
    return h % gs[0], (h // gs[0]) % gs[1], h // (gs[0] * gs[1])


def wave_model(hash_, cell_start, cell_end, b_cell_start, params, n):
    """Per wave of 64 consecutive sorted slots (arrays of length ceil(n / 64)):
    edge: an active lane sits in a grid-edge cell; hull: (nw, 9) hull lengths of the nine rows, row = 3 * (dz + 1) + (dy + 1)
    (zeros for an edge wave: the kernel forms none); plane: (nw, 3) their sums per z-plane; staged; wall_lanes: lanes with a
    non-empty boundary cell among their 27; lanes: active lanes.  `unstaged`: active particles in waves that do not stage."""
    gs = _grid(params)
    n = int(n)
    nw = (n + WAVE - 1) // WAVE
    cs_tab = np.asarray(cell_start).astype(np.int64)
    ce_tab = np.asarray(cell_end).astype(np.int64)
    cx, cy, cz = _cells(np.asarray(hash_)[:n], gs)
    on_edge = (cx == 0) | (cx == gs[0] - 1) | (cy == 0) | (cy == gs[1] - 1) | (cz == 0) | (cz == gs[2] - 1)

    def per_wave(a, fill):
        out = np.full(nw * WAVE, fill, dtype=a.dtype)
        out[:n] = a
        return out.reshape(nw, WAVE)

    edge = per_wave(on_edge, False).any(axis=1)
    lanes = per_wave(np.ones(n, bool), False).sum(axis=1)
    hull = np.zeros((nw, 9), np.int64)
    inner = ~on_edge
    for r in range(9):
        dz, dy = r // 3 - 1, r % 3 - 1
        lo = np.zeros(n, np.int64)
        hi = np.zeros(n, np.int64)
        h0 = ((cz[inner] + dz) * gs[1] + (cy[inner] + dy)) * gs[0] + cx[inner] - 1
        s = np.stack([cs_tab[h0], cs_tab[h0 + 1], cs_tab[h0 + 2]], axis=1)
        e = np.stack([ce_tab[h0], ce_tab[h0 + 1], ce_tab[h0 + 2]], axis=1)
        full = s != EMPTY
        some = full.any(axis=1)
        first = np.argmax(full, axis=1)
        last = 2 - np.argmax(full[:, ::-1], axis=1)
        k = np.arange(len(h0))
        a = np.where(some, s[k, first], 0)
        b = np.where(some, e[k, last], 0)
        assert np.all((b >= a) & (b <= n)), "cell tables inconsistent with n"
        lo[inner], hi[inner] = a, b
        lo_w, hi_w = per_wave(lo, 0), per_wave(hi, 0)
        non_empty = lo_w != hi_w
        anyrow = non_empty.any(axis=1)
        f = np.argmax(non_empty, axis=1)
        l = WAVE - 1 - np.argmax(non_empty[:, ::-1], axis=1)
        w = np.arange(nw)
        hull[:, r] = np.where(anyrow & ~edge, hi_w[w, l] - lo_w[w, f], 0)
    plane = hull.reshape(nw, 3, 3).sum(axis=2)
    staged = ~edge & np.all(plane <= POOL, axis=1)
    wall = np.zeros(n, bool)
    if b_cell_start is not None:
        bs_tab = np.asarray(b_cell_start)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    hc = (((cz + dz) & (gs[2] - 1)) * gs[1] + ((cy + dy) & (gs[1] - 1))) * gs[0] + ((cx + dx) & (gs[0] - 1))
                    wall |= bs_tab[hc] != EMPTY
    wall_lanes = per_wave(wall, False).sum(axis=1)
    return dict(edge=edge, hull=hull, plane=plane, staged=staged, wall_lanes=wall_lanes, lanes=lanes,
                unstaged=int(lanes[~staged].sum()))


def _pairs_in_cells(first, last):
    """(owner, candidate) index pairs for per-owner candidate ranges [first, last)"""
    cnt = np.maximum(last - first, 0)
    owner = np.repeat(np.arange(len(first)), cnt)
    start = np.cumsum(cnt) - cnt
    cand = np.arange(int(cnt.sum())) - np.repeat(start, cnt) + np.repeat(first, cnt)
    return owner, cand


def hit_counts(spos, hash_, cell_start, cell_end, params, n, b_cell_start=None, b_cell_end=None, sb=None):
    """Exact hit counts of every sorted slot over its 27 cells (power-of-two wrap, cell by cell): nf fluid candidates other than the
    slot itself with d2 < lenLtIr, nb boundary candidates with d2 < r2LeH2, d2 = (dx*dx + dy*dy) + dz*dz in float on the float
    differences, as the device's dot().  Returns (nf, nb) as int64 arrays."""
    gs = _grid(params)
    n = int(n)
    f = np.float32
    t_f, t_b = make_thresholds(np.asarray(params["interactionRadius"]).reshape(-1)[0])
    p = np.asarray(spos)[:n, :3].astype(f)
    cx, cy, cz = _cells(np.asarray(hash_)[:n], gs)
    nf = np.zeros(n, np.int64)
    nb = np.zeros(n, np.int64)

    def count(tab_s, tab_e, src, thr, skip_self):
        out = np.zeros(n, np.int64)
        s_all, e_all = np.asarray(tab_s).astype(np.int64), np.asarray(tab_e).astype(np.int64)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    hc = (((cz + dz) & (gs[2] - 1)) * gs[1] + ((cy + dy) & (gs[1] - 1))) * gs[0] + ((cx + dx) & (gs[0] - 1))
                    s = s_all[hc]
                    e = np.where(s == EMPTY, 0, e_all[hc])
                    s = np.where(s == EMPTY, 0, s)
                    i, j = _pairs_in_cells(s, e)
                    with np.errstate(invalid="ignore", over="ignore"):
                        d = p[i] - src[j]
                        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                        hit = d2 < thr
                    assert d2.dtype == f
                    if skip_self:
                        hit &= i != j
                    out += np.bincount(i[hit], minlength=n)
        return out

    nf = count(cell_start, cell_end, p, t_f, True)
    if sb is not None and len(sb):
        nb = count(b_cell_start, b_cell_end, np.asarray(sb)[:, :3].astype(f), t_b, False)
    return nf, nb


def predict(spos, hash_, cell_start, cell_end, params, n, b_cell_start=None, b_cell_end=None, sb=None):
    """wave_model + hit_counts + the three statistics of the staged launch with shared lists: STAT_UNSTAGED (active particles in
    waves that took the global-memory scan), STAT_HIT_OVERFLOW (nf + nb > HIT_CAP, or a non-finite owner) and STAT_HIT_MAX (the
    longest list that did not overflow)."""
    n = int(n)
    m = wave_model(hash_, cell_start, cell_end, b_cell_start if sb is not None and len(sb) else None, params, n)
    nf, nb = hit_counts(spos, hash_, cell_start, cell_end, params, n, b_cell_start, b_cell_end, sb)
    finite = np.all(np.isfinite(np.asarray(spos)[:n, :3]), axis=1)
    over = (nf + nb > HIT_CAP) | ~finite
    tot = (nf + nb)[~over]
    m.update(nf=nf, nb=nb, over=over, particle_staged=np.repeat(m["staged"], WAVE)[:n], particle_wall_lanes=np.repeat(m["wall_lanes"], WAVE)[:n],
             stat_unstaged=m["unstaged"], stat_hit_overflow=int(over.sum()), stat_hit_max=int(tot.max()) if len(tot) else 0)
    return m


# ---- the targeted scenes of tests/test_staged_scan_gpu.py (built here so that tests/test_staged_model_cpu.py can show, on the model
# alone, that each contains the branch it is named for) ---------------------------------------------------------------------------
def scene_params(grid, cell_over_h=1.0):
    """fp32 Muller SESPH defaults on a `grid` (three powers of two >= 4) of cells `cell_over_h` x h with its origin at 0"""
    from tests.oracle_lib import SESPH, Oracle

    p = Oracle.default_params(SESPH)
    h = np.float32(p["interactionRadius"][0])
    p["gridSize"][0] = grid
    p["numCells"][0] = grid[0] * grid[1] * grid[2]
    p["worldOrigin"][0] = (0.0, 0.0, 0.0)
    p["cellSize"][0] = np.float32(cell_over_h) * h
    return p


def _pts(xyz):
    a = np.ones((len(xyz), 4), np.float32)
    a[:, :3] = np.asarray(xyz, np.float64).astype(np.float32)
    return a


def _in_cells(rng, cells, per_cell, cell, lo=0.05, hi=0.95):
    """`per_cell` uniform points in each of `cells` (integer cell coordinates), `cell` metres per cell, away from the faces"""
    out = [(np.asarray(c, np.float64) + rng.uniform(lo, hi, (k, 3))) * cell for c, k in zip(cells, np.broadcast_to(per_cell, len(cells)))]
    return np.concatenate(out)


def _lattice(rng, lo, hi, spacing, h, jitter=0.05):
    """jittered lattice over [lo, hi) cells of size h at `spacing` x h"""
    ax = [np.arange(lo[a] + 0.1, hi[a] - 0.05, spacing) for a in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    return (g + rng.uniform(-jitter, jitter, g.shape)) * h


def _volumes(rng, nb):
    return rng.uniform(1e-5, 4e-5, nb).astype(np.float32)


def point_at_cutoff(b, ir):
    """a float position a, about ir in +x of the float position b, whose float squared distance to b — (dx*dx + dy*dy) + dz*dz on the
    float differences — is EXACTLY lenLtIr: the one value below r2LeH2 and not below lenLtIr, where the two cut-offs differ"""
    f = np.float32
    b = np.asarray(b, f)
    t_f, t_b = make_thresholds(ir)
    assert np.nextafter(t_f, f(1)) == t_b
    ax = f(b[0] + f(ir))
    xs = (ax + np.arange(-300, 300).astype(f) * np.spacing(ax)).astype(f)
    ys = (b[1] + np.arange(0, 4000).astype(f) * np.spacing(b[1]) * f(8)).astype(f)
    x, y = np.meshgrid(xs, ys, indexing="ij")
    dx, dy = x - b[0], y - b[1]
    d2 = (dx * dx + dy * dy) + f(0)
    i, j = np.argwhere(d2 == t_f)[0]
    return np.array([xs[i], ys[j], b[2]], f)


def targeted_scenes():
    """{name: dict(p, pos, vel, bi, vbi)}: bi / vbi None without walls.  Velocities are random (the viscosity terms are not
    zero).  Every scene is deterministic (seeded)."""
    rng = np.random.default_rng(20260)
    sc = {}

    def add(name, p, pos, bi=None):
        pos = _pts(pos)
        vel = np.zeros_like(pos)
        vel[:, :3] = rng.normal(0, 0.3, (len(pos), 3)).astype(np.float32)
        b = None if bi is None else _pts(bi)
        sc[name] = dict(p=p, pos=pos, vel=vel, bi=b, vbi=None if b is None else _volumes(rng, len(b)))

    p8 = scene_params((8, 8, 8))
    h = float(p8["interactionRadius"][0])
    # a small sheet of wall particles under the cloud of the tail scenes (cells z = 1, the cloud fills cells 2..5)
    sheet = np.stack(np.meshgrid(np.arange(2.1, 5.9, 0.45), np.arange(2.1, 5.9, 0.45), [1.8], indexing="ij"), -1).reshape(-1, 3) * h
    for n in (1, 63, 64, 65, 129):
        cloud = (2.0 + rng.uniform(0.05, 3.95, (n, 3))) * h
        add("tail%d" % n, p8, cloud)
        add("tail%d_walls" % n, p8, cloud, sheet)
    # edge and wrap fallback: one jittered block (cells 2..5 in x and y, 1..6 in z: all interior), shifted one cell up in z (cells
    # 2..7: the top plane is an edge), and shifted half out of the grid in z (wraps to cells 5, 6, 7, 0, 1, 2)
    block = _lattice(rng, (2, 2, 1), (6, 6, 7), 0.75, h)
    floor = np.stack(np.meshgrid(np.arange(2.05, 5.95, 0.5), np.arange(2.05, 5.95, 0.5), [1.02], indexing="ij"), -1).reshape(-1, 3) * h
    for name, dz in (("block_interior", 0.0), ("block_edge", 1.0), ("block_wrap", 4.0)):
        add(name, p8, block + np.array([0.0, 0.0, dz]) * h)
        add(name + "_walls", p8, block + np.array([0.0, 0.0, dz]) * h, floor + np.array([0.0, 0.0, dz]) * h)
    # hull lengths: cells of 3 h, so that 50 particles per cell are ~8 hits per particle (lists that do not overflow are what
    # the staging is checked through) — one x-row of cells at 50 per cell, the eight other rows empty
    p3 = scene_params((8, 8, 8), 3.0)
    c3 = 3.0 * h
    add("hull_line", p3, _in_cells(rng, [(x, 3, 3) for x in range(1, 7)], 50, c3))
    # a sheet of cells (one z-plane) at 36 per cell: middle rows exceed the pool, the outer rows do not
    add("hull_sheet", p3, _in_cells(rng, [(x, y, 3) for y in range(1, 7) for x in range(1, 7)], 36, c3))
    # the pool exactly full: five cells of 64 particles (a plus sign in one z-plane): the wave of the centre cell has hulls
    # 64 + 192 + 64 = 320 = STG_POOL, its own row 192 (> 128), its x-neighbours' own rows 128
    add("hull_pool_full", p3, _in_cells(rng, [(3, 2, 3), (2, 3, 3), (3, 3, 3), (4, 3, 3), (3, 4, 3)], 64, c3))
    # list overflow inside staged waves: a crowded blob in loose surroundings (as the crowded scenes of tests/test_pcisph_gpu.py
    # _bitwise_scenes) in the interior of a 16^3 grid; with walls: a tight knot of wall particles at the blob's rim and a sparse
    # patch further out
    rng = np.random.default_rng(7)
    p16 = scene_params((16, 16, 16))
    ctr = np.array([8.3, 8.4, 7.6]) * h
    crowd = np.concatenate([ctr + rng.uniform(-0.3 * h, 0.3 * h, (40, 3)), ctr + rng.uniform(-2.5 * h, 2.5 * h, (150, 3))])
    knot = np.concatenate([ctr + np.array([1.2, 0.1, 0.0]) * h + rng.uniform(-0.15 * h, 0.15 * h, (30, 3)),
                           ctr + np.array([-1.5, 1.0, 0.5]) * h + rng.uniform(-0.5 * h, 0.5 * h, (6, 3))])
    add("crowd", p16, crowd)
    add("crowd_walls", p16, crowd, knot)
    # wall sweep: a block in cells 2..5 with two more particles in the corner of cell (5,5,5) and one in the corner of cell (5,5,2);
    # a tight knot of 40 wall particles in cell (6,6,6) (its only fluid neighbours: the first two; their lists overflow with the
    # boundary hits below the fluid hits) and 4 wall particles in cell (6,6,1) (the third: a list that does not overflow)
    small = np.concatenate([_lattice(rng, (2, 2, 2), (6, 6, 6), 0.8, h), np.array([[5.8, 5.8, 5.8], [5.6, 5.7, 5.8], [5.8, 5.8, 2.2]]) * h])
    patch = np.concatenate([(6.02 + rng.uniform(0, 0.13, (40, 3))) * h, (np.array([6.03, 6.03, 1.88]) + rng.uniform(0, 0.08, (4, 3))) * h])
    add("wall_patch", p8, small, patch)
    # a floor sheet under the block: every lane of the lowest layer has wall cells
    add("wall_floor", p8, small, np.stack(np.meshgrid(np.arange(1.1, 6.9, 0.5), np.arange(1.1, 6.9, 0.5), [1.7], indexing="ij"), -1).reshape(-1, 3) * h)
    # FAST 11-bit offsets: ONE boundary cell with 2100 particles (> 2048), once diagonal to the block's corner cell (<= 4 wall
    # lanes in the wave: cooperative sweep) and once under the block (more: per-lane sweep); the particles fill the part of the
    # cell away from the fluid so that no list counts 1024 boundary hits (pack_counts: nb << 8 would reach a diagnostic bit)
    add("b2100_coop", p8, small, (6.0 + rng.uniform(0.05, 0.95, (2100, 3))) * h)
    add("b2100_lane", p8, small, (np.array([3.0, 3.0, 1.0]) + rng.uniform(0.05, 0.95, (2100, 3)) * np.array([1.0, 1.0, 0.3])) * h)
    # the two cut-offs: a wall particle at a float squared distance of exactly lenLtIr from a fluid particle is a hit of the shared
    # lists (d2 < r2LeH2) and its owner's is the longest list of the scene; with the three other particles of the owner's cell as the
    # only other wall lanes (cooperative sweep), and with four more in other cells around the wall particle's (per-lane sweep)
    wall = np.array([3.2, 3.5, 3.5], np.float32) * np.float32(h)
    owner = point_at_cutoff(wall, p8["interactionRadius"][0])
    near = np.concatenate([[owner], owner + np.array([[0.3, 0.2, 0.2], [0.35, -0.2, 0.1], [0.4, 0.05, -0.25]]) * h])
    more = np.array([[4.6, 4.6, 2.4], [3.3, 4.6, 2.4], [4.6, 2.4, 2.4], [3.3, 2.4, 2.4]]) * h   # (each alone)
    add("cut_pair_coop", p8, near, wall[None, :])
    add("cut_pair_lane", p8, np.concatenate([near, more]), wall[None, :])
    return sc


_oracle_cache = {}


def oracle_state(name, s):
    """The CPU oracle's partial step (fp32, tait = double7: the device's Tait convention) on a scene: the sorted state and tables
    the model reads, and density / pressure / forces.  Computed once per scene name."""
    if name in _oracle_cache:
        return _oracle_cache[name]
    import os

    from tests.oracle_lib import SESPH, STOP_FORCES, Oracle

    o = Oracle(s["p"], solver=SESPH, threads=min(16, os.cpu_count() or 1), tait="double7")
    o.set_particles(s["pos"], s["vel"])
    o.set_boundaries(s["bi"], s["vbi"], update_grid=False)
    o.step(1, stop=STOP_FORCES)
    names = ["hash", "index", "cellStart", "cellEnd", "sortedPos", "dens", "pres", "forces"]
    if s["bi"] is not None:
        names += ["bCellStart", "bCellEnd", "sbi"]
    st = {k: o.get(k) for k in names}
    st["params"] = o.params
    _oracle_cache[name] = st
    return st


def predict_scene(name, s):
    st = oracle_state(name, s)
    return predict(st["sortedPos"], st["hash"], st["cellStart"], st["cellEnd"], st["params"], len(s["pos"]),
                   st.get("bCellStart"), st.get("bCellEnd"), st.get("sbi"))
