// nrs_host_inflow.h — the host decisions of the sources and sinks (include/nereus_hip.h "sources and sinks"; DESIGN.md "Sources and
// sinks"), written once: which emitters, sink configurations and calls are accepted and the refusal texts; the emitter's frame, spacing,
// site counts and the rows of a disc; the schedule of a step with the capacity and max_particles rule; the bounds of a cull in the
// build's precision and the predicate itself.  No HIP: the kernels (nrs_kernels_inflow.h), the owner of the device buffers
// (InflowSystem, nrs_inflow.h) and a plain host program (tests/host_inflow_main.cpp) call the same routines; NRS_INF_HD is empty
// without hipcc.
//
// The arithmetic is part of the interface (the numpy model of the tests follows it bit for bit): doubles, in the order written, no
// contraction; sqrt, cbrt and floor are the C library's.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "nrs_host_sample.h"

#if defined(__HIPCC__)
#define NRS_INF_HD __host__ __device__ inline
#else
#define NRS_INF_HD inline
#endif

namespace nrs {

constexpr uint64_t INFLOW_MAX_LAYER_SITES = 1ull << 24;
constexpr uint32_t INFLOW_MAX_HALF = 1u << 12;      // (2 k + 1)^2 <= 2^24 sites means k < 2^11; anything above this is refused early
constexpr uint32_t INFLOW_LAYERS_PER_LAUNCH = 8;    // layer origins travel as kernel arguments

// ---- the frame: d normalised, e1 = normalised d x axis (axis of d's smallest absolute component, lowest on a tie), e2 = d x e1 ------------
struct InflowFrame { double d[3], e1[3], e2[3]; };
static inline void inflow_cross(const double a[3], const double b[3], double c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
static inline double inflow_length(const double a[3]) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
// false: the direction has no length (or its length is not finite)
static inline bool inflow_frame(const double dir[3], InflowFrame &f)
{
    const double l = inflow_length(dir);
    if (!(l > 0.0) || !std::isfinite(l)) return false;
    for (int a = 0; a < 3; ++a) f.d[a] = dir[a] / l;
    const double ax = std::fabs(f.d[0]), ay = std::fabs(f.d[1]), az = std::fabs(f.d[2]);
    double axis[3] = {0.0, 0.0, 0.0};
    if (ax <= ay && ax <= az) axis[0] = 1.0;
    else if (ay <= az) axis[1] = 1.0;
    else axis[2] = 1.0;
    double t[3];
    inflow_cross(f.d, axis, t);
    const double tl = inflow_length(t);
    for (int a = 0; a < 3; ++a) f.e1[a] = t[a] / tl;
    inflow_cross(f.d, f.e1, f.e2);
    return true;
}

// ---- the sites of a layer --------------------------------------------------------------------------------------------------------------
// rect: i in [-ku, ku], j in [-kv, kv].  disc: ku = kv = floor(r / s); row j keeps |i| <= half[j + kv] (-1: an empty row), the largest i
// with (i s)^2 + (j s)^2 <= r^2; start[j + kv]: sites in the rows before it.
struct InflowSites {
    uint32_t ku = 0, kv = 0;
    uint64_t sites = 0;
    std::vector<int32_t> half;   // disc only
    std::vector<uint32_t> start; // disc only
};
static inline double inflow_spacing(double given, double particleMass, double restDensity) { return given > 0.0 ? given : std::cbrt(particleMass / restDensity); }
// false: more than 2^24 sites (or a count that cannot be formed)
static inline bool inflow_sites(uint32_t shape, const double halfExtent[2], double s, InflowSites &o)
{
    o = InflowSites();
    const double fu = std::floor(halfExtent[0] / s), fv = std::floor((shape == NRS_EMITTER_DISC ? halfExtent[0] : halfExtent[1]) / s);
    if (!(fu >= 0.0 && fu <= (double)INFLOW_MAX_HALF) || !(fv >= 0.0 && fv <= (double)INFLOW_MAX_HALF)) return false;
    o.ku = (uint32_t)fu; o.kv = (uint32_t)fv;
    if (shape != NRS_EMITTER_DISC) {
        o.sites = (uint64_t)(2u * o.ku + 1u) * (2u * o.kv + 1u);
        return o.sites <= INFLOW_MAX_LAYER_SITES;
    }
    const double r = halfExtent[0], r2 = r * r;
    const int32_t k = (int32_t)o.ku;
    o.half.resize(2 * (size_t)k + 1);
    o.start.resize(2 * (size_t)k + 1);
    uint64_t total = 0;
    for (int32_t j = -k; j <= k; ++j) {
        const double js = (double)j * s, j2 = js * js;
        int32_t m = -1;
        for (int32_t i = 0; i <= k; ++i) {
            const double is = (double)i * s;
            if (is * is + j2 <= r2) m = i; else break;
        }
        o.half[j + k] = m;
        o.start[j + k] = (uint32_t)total;
        total += m < 0 ? 0u : 2u * (uint32_t)m + 1u;
    }
    o.sites = total;
    return total <= INFLOW_MAX_LAYER_SITES;
}

// site k of a layer as (i, j).  rect: i = k mod (2 ku + 1) - ku, j = k div (2 ku + 1) - kv.  disc: the row whose start is the last one
// <= k (binary search over the 2 kv + 1 rows; of rows with equal starts the last is the one that is not empty), i = k - start - half.
NRS_INF_HD void inflow_site(uint32_t k, uint32_t ku, uint32_t kv, bool disc, const int32_t *rowHalf, const uint32_t *rowStart, int32_t &i, int32_t &j)
{
    if (disc) {
        uint32_t lo = 0, hi = 2u * kv; // rows [lo, hi]; start[0] = 0 <= k
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1u) >> 1;
            if (rowStart[mid] <= k) lo = mid; else hi = mid - 1u;
        }
        j = (int32_t)lo - (int32_t)kv;
        i = (int32_t)(k - rowStart[lo]) - rowHalf[lo];
    } else {
        const uint32_t w = 2u * ku + 1u;
        i = (int32_t)(k % w) - (int32_t)ku;
        j = (int32_t)(k / w) - (int32_t)kv;
    }
}
// the position of site (i, j) of the layer with origin o: (R)(o[a] + (i s) e1[a] + (j s) e2[a]), double, in this order, no contraction
template <typename R> NRS_INF_HD void inflow_site_pos(const double o[3], const double e1[3], const double e2[3], double s, int32_t i, int32_t j, R x[3])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double is = (double)i * s, js = (double)j * s;
    for (int a = 0; a < 3; ++a) x[a] = (R)(o[a] + is * e1[a] + js * e2[a]);
}

// ---- an emitter: checked, then stored with its derived values ----------------------------------------------------------------------------
struct EmitterSlot {
    bool used = false;
    nrs_emitter e = {};   // as stored: direction normalised, spacing as given
    InflowFrame f = {};
    double s = 0.0;       // the spacing in use
    InflowSites sites;
    double acc = 0.0;
    uint64_t emitted = 0, dropped = 0;
    bool tableDirty = true; // (disc) the rows still have to reach the device
};
static inline int inflow_check_slot(uint32_t slot)
{
    if (slot >= (uint32_t)NRS_MAX_EMITTERS) return fail(NRS_E_INVALID, "emitter: slot must be below NRS_MAX_EMITTERS (16)");
    return NRS_OK;
}
// e checked against the current particleMass / restDensity; on success `out` is the slot to store
static inline int inflow_check_emitter(const nrs_emitter *e, double particleMass, double restDensity, EmitterSlot &out)
{
    if (e->shape != NRS_EMITTER_RECT && e->shape != NRS_EMITTER_DISC) return fail(NRS_E_INVALID, "emitter: shape must be NRS_EMITTER_RECT or NRS_EMITTER_DISC");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(e->center[a]) || !std::isfinite(e->direction[a])) return fail(NRS_E_INVALID, "emitter: center and direction must be finite");
    if (!std::isfinite(e->half_extent[0]) || !std::isfinite(e->half_extent[1]) || !std::isfinite(e->speed) || !std::isfinite(e->spacing))
        return fail(NRS_E_INVALID, "emitter: half_extent, speed and spacing must be finite");
    EmitterSlot o;
    if (!inflow_frame(e->direction, o.f)) return fail(NRS_E_INVALID, "emitter: direction has no length");
    if (e->speed < 0.0) return fail(NRS_E_INVALID, "emitter: speed must be >= 0");
    if (e->spacing < 0.0) return fail(NRS_E_INVALID, "emitter: spacing must be >= 0 (0: cbrt(particleMass / restDensity))");
    if (e->half_extent[0] < 0.0 || (e->shape == NRS_EMITTER_RECT && e->half_extent[1] < 0.0)) return fail(NRS_E_INVALID, "emitter: half_extent must be >= 0");
    o.s = inflow_spacing(e->spacing, particleMass, restDensity);
    if (!(o.s > 0.0) || !std::isfinite(o.s)) return fail(NRS_E_INVALID, "emitter: spacing 0 needs particleMass / restDensity > 0");
    if (!inflow_sites(e->shape, e->half_extent, o.s, o.sites)) return fail(NRS_E_INVALID, "emitter: spacing so small that a layer has more than 2^24 sites");
    o.used = true;
    o.e = *e;
    o.e.enabled = e->enabled ? 1u : 0u;
    for (int a = 0; a < 3; ++a) o.e.direction[a] = o.f.d[a];
    out = std::move(o);
    return NRS_OK;
}

// ---- the schedule of one step for one slot ------------------------------------------------------------------------------------------------
// acc += speed dt; every whole spacing gives a layer whose origin lies acc (after the subtraction) along d from the centre.  A layer
// that does not fit `room` whole, or would pass max_particles, is dropped; the accumulator advances all the same.  Appends the offsets
// of the layers that are emitted, in order; lowers `room`.
static inline void inflow_schedule(EmitterSlot &sl, double dt, uint64_t &room, std::vector<double> &offsets)
{
    if (!sl.used || !sl.e.enabled) return;
    sl.acc += sl.e.speed * dt;
    const uint64_t sites = sl.sites.sites;
    while (sl.acc >= sl.s) {
        sl.acc -= sl.s;
        const bool fits = sites <= room && (!sl.e.max_particles || sl.emitted + sites <= sl.e.max_particles);
        if (fits) {
            offsets.push_back(sl.acc);
            room -= sites;
            sl.emitted += sites;
        } else {
            sl.dropped += sites;
        }
    }
}
// the sites inflow_schedule would emit for this slot and step, with nothing changed but `room` (the same arithmetic on copies of the
// accumulator and the count): a tracked step asks before it hands out ids (nrs_ctx_impl.h)
static inline uint64_t inflow_schedule_count(const EmitterSlot &sl, double dt, uint64_t &room)
{
    if (!sl.used || !sl.e.enabled) return 0;
    double acc = sl.acc;
    acc += sl.e.speed * dt;
    const uint64_t sites = sl.sites.sites;
    uint64_t emitted = sl.emitted, total = 0;
    while (acc >= sl.s) {
        acc -= sl.s;
        if (sites <= room && (!sl.e.max_particles || emitted + sites <= sl.e.max_particles)) {
            room -= sites;
            emitted += sites;
            total += sites;
        }
    }
    return total;
}
static inline void inflow_origin(const EmitterSlot &sl, double offset, double o[3])
{
    for (int a = 0; a < 3; ++a) o[a] = sl.e.center[a] + offset * sl.f.d[a];
}

// ---- nrs_emit_block --------------------------------------------------------------------------------------------------------------------------
// the lattice and the velocity of nrs_emit_block and nrs_emit_mesh
static inline int inflow_check_sites(const nrs_lattice *L, const double *vel, uint64_t *nodes)
{
    NRSCHK(sample_check_lattice(L, nodes));
    if (!vel) return fail(NRS_E_INVALID, "emit block: vel is NULL");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(vel[a])) return fail(NRS_E_INVALID, "emit block: vel is not finite");
    return NRS_OK;
}
static inline int inflow_check_block(const nrs_lattice *L, const double *vel, uint64_t n, uint64_t cap, uint64_t *nodes)
{
    NRSCHK(inflow_check_sites(L, vel, nodes));
    if (*nodes > cap - n) return fail(NRS_E_CAPACITY, "emit block: the lattice has more nodes than capacity - n");
    return NRS_OK;
}

// ---- the sinks ---------------------------------------------------------------------------------------------------------------------------------
static inline int inflow_check_sinks(const nrs_sink_config *c)
{
    if (c->flags & ~(uint32_t)NRS_SINK_DOMAIN) return fail(NRS_E_INVALID, "sinks: flags has unknown bits");
    if (c->nboxes > (uint32_t)NRS_MAX_SINK_BOXES) return fail(NRS_E_INVALID, "sinks: nboxes above NRS_MAX_SINK_BOXES (16)");
    if (c->reserved) return fail(NRS_E_INVALID, "sinks: reserved must be 0");
    for (uint32_t b = 0; b < c->nboxes; ++b)
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(c->boxes[b][a]) || !std::isfinite(c->boxes[b][3 + a])) return fail(NRS_E_INVALID, "sinks: a box bound is not finite");
            if (!(c->boxes[b][a] < c->boxes[b][3 + a])) return fail(NRS_E_INVALID, "sinks: a box needs min < max on every axis");
        }
    return NRS_OK;
}
// the state both kinds of call are refused in; `driven`: the call also minds a host-driven IISPH step (nrs_cull, nrs_emit_block)
static inline int inflow_refusal(bool slab, bool midStep, bool iisphInProgress, bool driven)
{
    if (slab) return fail(NRS_E_INVALID, "sources and sinks on a slab context (its arrays hold halo copies)");
    if (midStep) return fail(NRS_E_STATE, "sources and sinks while the state is mid-update after nrs_step_partial");
    if (driven && iisphInProgress) return fail(NRS_E_STATE, "sources and sinks while a host-driven IISPH step is in progress (nrs_iisph_finish first)");
    return NRS_OK;
}
static inline int inflow_refuse_slab() { return fail(NRS_E_INVALID, "nrs_slab_configure on a context with sources or sinks"); }
// true when the step counted as k-th since nrs_sinks_set culls (interval 0 = 1): k = interval, 2 interval, ...
static inline bool inflow_cull_due(uint64_t k, uint32_t interval) { return k % (uint64_t)(interval ? interval : 1u) == 0; }

// the bounds of a cull as the kernels get them, in the build's precision (one rounding of every double)
template <typename R> struct CullBounds {
    R lo[3], hi[3];   // the domain, tested when `domain` is set
    R box[NRS_MAX_SINK_BOXES][6];
    uint32_t domain, nboxes;
};
template <typename R>
static inline CullBounds<R> inflow_bounds(const nrs_sink_config *c, const R worldOrigin[3], const uint32_t gridSize[3], const R cellSize[3])
{
    CullBounds<R> B;
    std::memset(&B, 0, sizeof(B));
    for (int a = 0; a < 3; ++a) {
        B.lo[a] = worldOrigin[a];
        B.hi[a] = (R)((double)worldOrigin[a] + (double)gridSize[a] * (double)cellSize[a]);
    }
    if (!c) return B;
    B.domain = (c->flags & NRS_SINK_DOMAIN) ? 1u : 0u;
    B.nboxes = c->nboxes;
    for (uint32_t b = 0; b < c->nboxes; ++b)
        for (int a = 0; a < 6; ++a) B.box[b][a] = (R)c->boxes[b][a];
    return B;
}
// true: the particle at (x, y, z) is removed
template <typename R> NRS_INF_HD bool inflow_caught(const CullBounds<R> &B, R x, R y, R z)
{
    if (!(x - x == (R)0) || !(y - y == (R)0) || !(z - z == (R)0)) return true; // NaN, +-inf
    if (B.domain && !(x >= B.lo[0] && x < B.hi[0] && y >= B.lo[1] && y < B.hi[1] && z >= B.lo[2] && z < B.hi[2])) return true;
    for (uint32_t b = 0; b < B.nboxes; ++b)
        if (x >= B.box[b][0] && x < B.box[b][3] && y >= B.box[b][1] && y < B.box[b][4] && z >= B.box[b][2] && z < B.box[b][5]) return true;
    return false;
}

} // namespace nrs
