"""A numpy restatement of the sources and sinks (include/nereus_hip.h "sources and sinks"; nereus_amd/csrc/nrs_host_inflow.h): the
emitter's frame, spacing, sites and schedule with the capacity and max_particles rule, the positions of emitted layers and of a lattice
block, the cull predicate and the order-keeping compaction.  Everything is float64 in the order the header states, rounded to the
build's SReal once, so the device's bytes can be compared with the model's.
"""
import math

import numpy as np

RECT, DISC = 0, 1
SINK_DOMAIN = 1
MAX_LAYER_SITES = 1 << 24


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float64)


def length(a):
    return math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def frame(direction):
    """(d, e1, e2): d normalised; e1 = normalised d x axis, axis of d's smallest absolute component (lowest on a tie); e2 = d x e1"""
    d = np.asarray(direction, np.float64)
    d = d / length(d)
    ax = np.abs(d)
    axis = np.zeros(3)
    if ax[0] <= ax[1] and ax[0] <= ax[2]:
        axis[0] = 1.0
    elif ax[1] <= ax[2]:
        axis[1] = 1.0
    else:
        axis[2] = 1.0
    t = cross(d, axis)
    e1 = t / length(t)
    return d, e1, cross(d, e1)


def spacing_of(given, params):
    if given > 0.0:
        return float(given)
    return float(np.cbrt(np.float64(params["particleMass"][0]) / np.float64(params["restDensity"][0])))


def sites(shape, half_extent, s):
    """the (i, j) of a layer, j-major, as an (m, 2) int64 array"""
    if shape == DISC:
        r = float(half_extent[0])
        k = int(math.floor(r / s))
        out = []
        for j in range(-k, k + 1):
            for i in range(-k, k + 1):
                if (i * s) * (i * s) + (j * s) * (j * s) <= r * r:
                    out.append((i, j))
        return np.array(out, np.int64).reshape(-1, 2)
    ku, kv = int(math.floor(half_extent[0] / s)), int(math.floor(half_extent[1] / s))
    jj, ii = np.meshgrid(np.arange(-kv, kv + 1), np.arange(-ku, ku + 1), indexing="ij")
    return np.stack([ii.ravel(), jj.ravel()], 1).astype(np.int64)


class Emitter:
    """one slot: the emitter as nrs_emitter_set stores it, its accumulator and counts"""

    def __init__(self, params, center, direction, half_extent, speed, spacing=0.0, shape=RECT, enabled=True, max_particles=0):
        self.center = np.asarray(center, np.float64)
        self.d, self.e1, self.e2 = frame(direction)
        self.shape, self.speed, self.enabled, self.max_particles = shape, float(speed), bool(enabled), int(max_particles)
        self.s = spacing_of(float(spacing), params)
        he = np.broadcast_to(np.asarray(half_extent, np.float64), (2,))
        self.ij = sites(shape, he, self.s)
        self.acc, self.emitted, self.dropped = 0.0, 0, 0

    def schedule(self, dt, room):
        """the offsets of the layers this step emits, given `room` free slots; advances the accumulator and the counts"""
        out = []
        if not self.enabled:
            return out
        self.acc += self.speed * dt
        m = len(self.ij)
        while self.acc >= self.s:
            self.acc -= self.s
            if m <= room and (not self.max_particles or self.emitted + m <= self.max_particles):
                out.append(self.acc)
                room -= m
                self.emitted += m
            else:
                self.dropped += m
        return out

    def layer(self, offset, real):
        """(pos4, vel4) of the layer whose origin lies `offset` along d from the centre"""
        o = self.center + offset * self.d
        i_s, j_s = self.ij[:, 0].astype(np.float64) * self.s, self.ij[:, 1].astype(np.float64) * self.s
        pos = np.ones((len(self.ij), 4), real)
        vel = np.zeros((len(self.ij), 4), real)
        for a in range(3):
            pos[:, a] = ((o[a] + i_s * self.e1[a]) + j_s * self.e2[a]).astype(real)
            vel[:, a] = real(self.speed * self.d[a])
        return pos, vel

    def step(self, dt, room, real):
        """the particles one step appends: (pos4, vel4), possibly empty"""
        parts = [self.layer(off, real) for off in self.schedule(dt, room)]
        if not parts:
            return np.zeros((0, 4), real), np.zeros((0, 4), real)
        return np.concatenate([p for p, _ in parts]), np.concatenate([v for _, v in parts])


def block(origin, spacing, dims, vel, real):
    """the nodes of a lattice in its linear index order ((k * dims[1] + j) * dims[0] + i) with velocity vel"""
    sp = np.broadcast_to(np.asarray(spacing, np.float64), (3,))
    k, j, i = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    idx = [i.ravel().astype(np.float64), j.ravel().astype(np.float64), k.ravel().astype(np.float64)]
    pos = np.ones((len(idx[0]), 4), real)
    v4 = np.zeros((len(idx[0]), 4), real)
    for a in range(3):
        pos[:, a] = (np.float64(origin[a]) + idx[a] * sp[a]).astype(real)
        v4[:, a] = real(vel[a])
    return pos, v4


def domain(params, real):
    """(lo, hi) of the grid box in SReal: hi formed in float64 from the parameters, rounded once"""
    lo = np.array([params["worldOrigin"][0][a] for a in range(3)], real)
    hi = np.array([np.float64(params["worldOrigin"][0][a]) + np.float64(params["gridSize"][0][a]) * np.float64(params["cellSize"][0][a]) for a in range(3)])
    return lo, hi.astype(real)


def caught(params, pos, real, boxes=(), domain_on=False):
    """the cull predicate per row of pos: a non-finite coordinate, (domain_on) outside the grid box, or inside a box"""
    x = np.asarray(pos, real)[:, :3]
    out = ~np.isfinite(x).all(axis=1)
    with np.errstate(invalid="ignore"):
        if domain_on:
            lo, hi = domain(params, real)
            out |= ~((x >= lo) & (x < hi)).all(axis=1)
        for b in np.asarray(boxes, np.float64).reshape(-1, 6):
            bb = b.astype(real)
            out |= ((x >= bb[:3]) & (x < bb[3:])).all(axis=1)
    return out


def compact(gone, *arrays):
    """the survivors of every array, in order"""
    keep = ~gone
    return [None if a is None else a[keep] for a in arrays]


def cull_due(k, interval):
    """whether the k-th step (1-based) since the sinks were set culls"""
    return k % (interval if interval else 1) == 0
