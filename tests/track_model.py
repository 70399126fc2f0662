"""A numpy restatement of particle tracking (include/nereus_hip.h "particle identity and attributes"; nereus_amd/csrc/nrs_host_track.h,
nrs_kernels_track.h): how id, birth and the attribute record move through a step, an emission, a cull, an upload and a count change;
the id accounting; the inverse map of nrs_track_locate; and nrs_track_diffuse in exactly the device's order of operations, so that the
device's bytes can be compared with the model's.

Emission and the cull are built on tests/inflow_model.py (the schedule, the sites, the predicate, the compaction).  The diffusion takes
its smoothing-kernel terms from tests/sample_model.py (and through it tests/pcisph_model.py, pinned to the reference), and the
sampler's sorted order, the walk's pair order and the sequential sum from tests/diffuse_model.py.  The density the weights divide by is
the field sampler's density AT the particles, summed as the device sums it: one accumulator in the build's precision, the cells of the
27-cell walk z, y, x ascending, a cell's boundary particles after its fluid particles (sample_model.sample sums in float64 for its
error bound; a byte comparison needs the device's own order, which is what density() below restates with sample_model's terms).
"""
import numpy as np

from tests import diffuse_model as dm
from tests import inflow_model as im
from tests import pcisph_model as pm
from tests import sample_model as sm

NONE = 0xFFFFFFFF
LAST_ID = 0xFFFFFFFE
ATTR = 1
MAX_LOCATE = 1 << 27
U32 = np.uint32


class Exhausted(Exception):
    """the call would pass the last id (NRS_E_CAPACITY on the device); nothing was changed"""


def birth_of(steps_done):
    return min(int(steps_done), 0xFFFFFFFF)


# ---- the moves, as functions on arrays ------------------------------------------------------------------------------------------------------------
def step(ids, birth, rec, index):
    """behind a step's reorder: sorted slot s holds the particle that was at index[s]"""
    index = np.asarray(index, np.int64)
    return ids[index], birth[index], (None if rec is None else rec[index])


def append(ids, birth, rec, next_id, count, steps_done, value):
    """`count` new particles behind the living ones: consecutive ids from next_id, born now, the record `value`; -> (ids, birth, rec, next_id)"""
    count = int(count)
    if count and next_id + count - 1 > LAST_ID:
        raise Exhausted()
    ids = np.concatenate([ids, (next_id + np.arange(count, dtype=np.int64)).astype(U32)])
    birth = np.concatenate([birth, np.full(count, birth_of(steps_done), U32)])
    if rec is not None:
        rec = np.concatenate([rec, np.tile(np.asarray(value, np.float64).astype(rec.dtype), (count, 1))])
    return ids, birth, rec, next_id + count


def emit(ids, birth, rec, next_id, emitter, dt, room, steps_done, value):
    """the layers an inflow_model.Emitter schedules for this step (its accumulator and counts advance), layer-major, site order inside a
    layer; -> (ids, birth, rec, next_id, particles appended)"""
    m = len(emitter.ij) * len(emitter.schedule(dt, room))
    return append(ids, birth, rec, next_id, m, steps_done, value) + (m,)


def cull(params, pos, ids, birth, rec, real, boxes=(), domain_on=False):
    """inflow_model's predicate on pos and its order-keeping compaction of the tracked arrays; -> (ids, birth, rec, gone)"""
    gone = im.caught(params, pos, real, boxes=boxes, domain_on=domain_on)
    a, b, c = im.compact(gone, ids, birth, rec)
    return a, b, c, gone


def locate(ids, first, count):
    """slot_of[k] = the slot of id first + k, NONE where it does not live"""
    out = np.full(int(count), NONE, U32)
    k = np.asarray(ids, np.int64) - int(first)
    ok = (k >= 0) & (k < int(count))
    out[k[ok]] = np.nonzero(ok)[0].astype(U32)
    return out


# ---- a tracked context's bookkeeping: the functions above with the host rules of nrs_host_track.h --------------------------------------------------
class State:
    def __init__(self, n, real=np.float32, attr=True):
        self.real, self.attr = real, attr
        self.enable(n)

    def enable(self, n):
        self.ids = np.arange(n, dtype=U32)
        self.birth = np.zeros(n, U32)
        self.rec = np.zeros((n, 4), self.real) if self.attr else None
        self.next_id, self.steps = int(n), 0
        self.values = {s: np.zeros(4) for s in range(-1, 16)}

    @property
    def n(self):
        return len(self.ids)

    def step(self, index):
        self.ids, self.birth, self.rec = step(self.ids, self.birth, self.rec, index)
        self.steps += 1

    def append(self, count, slot=-1):
        self.ids, self.birth, self.rec, self.next_id = append(self.ids, self.birth, self.rec, self.next_id, count, self.steps, self.values[slot])

    def emit(self, emitter, dt, room, slot):
        *arrays, m = emit(self.ids, self.birth, self.rec, self.next_id, emitter, dt, room, self.steps, self.values[slot])
        self.ids, self.birth, self.rec, self.next_id = arrays
        return m

    def cull(self, params, pos, boxes=(), domain_on=False):
        self.ids, self.birth, self.rec, gone = cull(params, pos, self.ids, self.birth, self.rec, self.real, boxes, domain_on)
        return gone

    def upload(self, first, count):
        """nrs_upload_particles(first, count): slots at or above the old n are new"""
        if first + count > self.n:
            self.append(first + count - self.n)

    def set_n(self, nn):
        if nn > self.n:
            self.append(nn - self.n)
        else:
            self.ids, self.birth = self.ids[:nn], self.birth[:nn]
            self.rec = None if self.rec is None else self.rec[:nn]

    def upload_ids(self, ids, first=0):
        ids = np.asarray(ids, U32)
        assert not (ids == NONE).any() and first + len(ids) <= self.n
        self.ids = self.ids.copy()
        self.ids[first:first + len(ids)] = ids
        if len(ids):
            self.next_id = max(self.next_id, int(ids.max()) + 1)


# ---- nrs_track_diffuse --------------------------------------------------------------------------------------------------------------------------------
def _keys(params, x, y, i, j, real):
    """the walk's cell number 0 .. 26 (z, y, x ascending) of y_j seen from x_i"""
    off = dm.cells(params, y, real)[j] - dm.cells(params, x, real)[i]
    return ((off[:, 2] + 1) * 3 + (off[:, 1] + 1)) * 3 + (off[:, 0] + 1)


def density(params, sx, kernel_set=pm.MULLER, walls=None):
    """the sampler's NRS_FIELD_DENSITY (| NRS_FIELD_WALLS with walls = NRS_ARR_B_SORTED) at the sorted particles sx themselves, summed as
    the device sums: one accumulator in the build's precision, cell by cell, fluid before walls inside a cell"""
    real = pm.real_of(params)
    m0, rd = real(pm._p(params, "particleMass")), real(pm._p(params, "restDensity"))
    n = len(sx)
    i, j, d = dm.walk_pairs(params, sx, sx, real)
    t = (m0 * sm._w(params, d, kernel_set, real)).astype(real)
    if walls is None or not len(walls):
        return dm.seq_sum(n, i, t, real)
    b = np.asarray(walls).astype(real)
    ib, jb, db = dm.walk_pairs(params, sx, b[:, :3], real)
    psi = (rd * b[jb, 3]).astype(real)
    tb = (psi * sm._w(params, db, kernel_set, real)).astype(real)
    ii, jj = np.concatenate([i, ib]), np.concatenate([j, jb])
    key = np.concatenate([_keys(params, sx, sx, i, j, real), _keys(params, sx, b[:, :3], ib, jb, real)])
    kind = np.concatenate([np.zeros(len(i), np.int64), np.ones(len(ib), np.int64)])
    o = np.lexsort((jj, kind, key, ii))
    return dm.seq_sum(n, ii[o], np.concatenate([t, tb])[o], real)


def weights(params, pos, kernel_set=pm.MULLER, walls=None):
    """(order, i, j, w): the sampler's sorted order of pos and, in the walk's order, the pairs (sorted slots i, j != i, 0 < length < h)
    with the weight w_ij of the Laplacian in the build's precision"""
    real = pm.real_of(params)
    h, m0 = real(pm._p(params, "interactionRadius")), real(pm._p(params, "particleMass"))
    order = dm.sorted_order(params, pos, real)
    sx = np.asarray(pos)[order, :3].astype(real)
    fin = np.isfinite(sx.astype(np.float64)).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        rho = density(params, sx, kernel_set, walls)
        i, j, d = dm.walk_pairs(params, sx, sx, real, same=True)
    ln = pm._len(d)
    keep = (ln != 0) & fin[i]
    i, j, d, ln = i[keep], j[keep], d[keep], ln[keep]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = sm._gw(params, d, kernel_set, real)
        dot = d[:, 0] * g[:, 0] + d[:, 1] * g[:, 1] + d[:, 2] * g[:, 2]
        r = ln.astype(real)
        eta2 = real(0.01) * (h * h)
        w = (m0 / (rho[i] * rho[j])) * (dot / (r * r + eta2))
    assert w.dtype == real and dot.dtype == real
    return order, i, j, w


def diffuse(params, pos, rec, kappa, dt, ks=pm.MULLER, walls=None, info=None):
    """one nrs_track_diffuse on the record rec (n, 4) of the particles at pos (both in the current order); dt must be the step to take
    (the context's timestep for the device's dt == 0); info, a dict, receives kmax (the largest neighbour count) and the pairs"""
    real = pm.real_of(params)
    rho0 = real(pm._p(params, "restDensity"))
    rec = np.asarray(rec, real)
    order, i, j, w = weights(params, pos, ks, walls)
    n = len(order)
    a = rec[order]
    new = a.copy()
    for c in range(4):
        if float(kappa[c]) == 0.0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            acc = dm.seq_sum(n, i, (a[i, c] - a[j, c]) * w, real)
            new[:, c] = a[:, c] + (((real(2) * real(dt)) * real(kappa[c])) * rho0) * acc
    fin = np.isfinite(np.asarray(pos)[order, :3].astype(np.float64)).all(axis=1)
    new[~fin] = a[~fin]   # "a particle with a non-finite position keeps its record": its bytes, not a + 0
    out = rec.copy()
    out[order] = new
    if info is not None:
        info.update(kmax=int(np.bincount(i, minlength=n).max()) if len(i) else 0, order=order, i=i, j=j, w=w)
    return out


def stability(params, pos, kappa, dt, ks=pm.MULLER, walls=None):
    """max_i lambda_i = 2 dt kappa rho0 sum_j |w_ij| (float64 of the device's weights), kappa the largest coefficient: at most 1 for a
    step that obeys the maximum principle"""
    order, i, j, w = weights(params, pos, ks, walls)
    s = np.bincount(i, weights=np.abs(w.astype(np.float64)), minlength=len(order))
    return float(2.0 * float(dt) * float(np.max(kappa)) * pm._p(params, "restDensity") * s.max())
