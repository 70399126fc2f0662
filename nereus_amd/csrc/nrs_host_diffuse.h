// nrs_host_diffuse.h — the host decisions of the diffuse particles (include/nereus_hip.h "diffuse particles"; DESIGN.md "Diffuse
// particles") and the per-particle rules, written once: which configurations and calls are accepted, when a context refuses, how many
// bytes a result takes and which result an id means; the counter-based hash behind every uniform draw; the clamp of a potential and the
// number of births; the birth of one diffuse particle; the advection of one.  No HIP: the kernels (nrs_kernels_diffuse.h) and a plain
// host program (tests/host_diffuse_main.cpp) call the same routines; NRS_DIFF_HD is empty without hipcc.
//
// The arithmetic of the routines is part of the interface (the numpy model of the tests follows it bit for bit): SReal sums, products
// and quotients in the order written, no contraction; every length is the library's float length() — the float square root of the
// dot product rounded to float, also in an fp64 build.
#pragma once
#include <cmath>
#include <cstdint>

#include "nrs_host_sample.h"

#if defined(__HIPCC__)
#define NRS_DIFF_HD __host__ __device__ inline
#else
#define NRS_DIFF_HD inline
#endif

namespace nrs {

constexpr uint32_t DIFFUSE_MAX_CAPACITY = 1u << 30;       // offsets and launch indices are 32-bit
constexpr uint32_t DIFFUSE_MAX_PER_PARTICLE = 1u << 10;   // births per fluid particle per step
constexpr uint64_t DIFFUSE_MAX_BIRTHS = 1ull << 31;       // N * max_per_particle: the scanned offsets are 32-bit
constexpr uint32_t DIFFUSE_DRAWS_PER_BIRTH = 10;          // four pairs for the disc, X_h, X_l
constexpr uint32_t DIFFUSE_RESULTS = 6;

// ---- the configuration -------------------------------------------------------------------------------------------------------------
static inline bool diffuse_range_ok(const double r[2]) { return std::isfinite(r[0]) && std::isfinite(r[1]) && r[0] < r[1]; }
static inline int diffuse_check_config(const nrs_diffuse_config *c)
{
    if (!c) return fail(NRS_E_INVALID, "diffuse config is NULL");
    if (c->struct_size != sizeof(nrs_diffuse_config)) return fail(NRS_E_INVALID, "diffuse config: struct_size is not sizeof(nrs_diffuse_config)");
    if (!c->capacity) return fail(NRS_E_INVALID, "diffuse config: capacity of 0");
    if (c->capacity > DIFFUSE_MAX_CAPACITY) return fail(NRS_E_INVALID, "diffuse config: capacity above 2^30");
    if (!diffuse_range_ok(c->tau_ta)) return fail(NRS_E_INVALID, "diffuse config: tau_ta must be finite with min < max");
    if (!diffuse_range_ok(c->tau_wc)) return fail(NRS_E_INVALID, "diffuse config: tau_wc must be finite with min < max");
    if (!diffuse_range_ok(c->tau_k)) return fail(NRS_E_INVALID, "diffuse config: tau_k must be finite with min < max");
    if (!std::isfinite(c->k_ta) || c->k_ta < 0.0) return fail(NRS_E_INVALID, "diffuse config: k_ta must be finite and >= 0");
    if (!std::isfinite(c->k_wc) || c->k_wc < 0.0) return fail(NRS_E_INVALID, "diffuse config: k_wc must be finite and >= 0");
    if (!std::isfinite(c->lifetime[0]) || !std::isfinite(c->lifetime[1]) || c->lifetime[0] < 0.0 || c->lifetime[0] > c->lifetime[1])
        return fail(NRS_E_INVALID, "diffuse config: lifetime must be finite with 0 <= min <= max");
    if (!std::isfinite(c->k_buoyancy)) return fail(NRS_E_INVALID, "diffuse config: k_buoyancy is not finite");
    if (!(c->k_drag >= 0.0 && c->k_drag <= 1.0)) return fail(NRS_E_INVALID, "diffuse config: k_drag must lie in [0, 1]");
    if (c->max_per_particle < 1u || c->max_per_particle > DIFFUSE_MAX_PER_PARTICLE)
        return fail(NRS_E_INVALID, "diffuse config: max_per_particle must lie in [1, 1024]");
    if (c->reserved) return fail(NRS_E_INVALID, "diffuse config: reserved must be 0");
    return NRS_OK;
}

// the configuration as the kernels get it, in the build's precision (one rounding of every double)
template <typename R> struct DiffuseCfg {
    uint64_t seed;
    R taMin, taMax, wcMin, wcMax, kMin, kMax; // clamp ranges
    R kTa, kWc;
    R lifeMin, lifeMax;
    R kBuoyancy, kDrag;
    uint32_t sprayBelow, bubbleAbove, maxPer, capacity;
};
template <typename R> static inline DiffuseCfg<R> diffuse_cfg(const nrs_diffuse_config &c)
{
    DiffuseCfg<R> d;
    d.seed = c.seed;
    d.taMin = (R)c.tau_ta[0]; d.taMax = (R)c.tau_ta[1];
    d.wcMin = (R)c.tau_wc[0]; d.wcMax = (R)c.tau_wc[1];
    d.kMin = (R)c.tau_k[0]; d.kMax = (R)c.tau_k[1];
    d.kTa = (R)c.k_ta; d.kWc = (R)c.k_wc;
    d.lifeMin = (R)c.lifetime[0]; d.lifeMax = (R)c.lifetime[1];
    d.kBuoyancy = (R)c.k_buoyancy; d.kDrag = (R)c.k_drag;
    d.sprayBelow = c.spray_below; d.bubbleAbove = c.bubble_above; d.maxPer = c.max_per_particle; d.capacity = c.capacity;
    return d;
}

// ---- when a call is refused: what is wrong with the argument comes before what is wrong with the state ---------------------------------
static inline int diffuse_check_dt(double dt)
{
    if (!(dt >= 0.0) || !std::isfinite(dt)) return fail(NRS_E_INVALID, "diffuse step: dt must be finite and >= 0 (0: the context's timestep)");
    return NRS_OK;
}
// the sampler's facts (nrs_host_sample.h) with the diffuse particles' texts; `configured`: nrs_diffuse_configure has succeeded
static inline int diffuse_refusal(const SampleFacts &f, bool configured)
{
    if (f.slab) return fail(NRS_E_INVALID, "diffuse particles on a slab context (its arrays hold halo copies)");
    if (!configured) return fail(NRS_E_STATE, "diffuse particles before nrs_diffuse_configure");
    if (f.midStep) return fail(NRS_E_STATE, "diffuse particles while the state is mid-update after nrs_step_partial");
    if (f.iisphInProgress) return fail(NRS_E_STATE, "diffuse particles while a host-driven IISPH step is in progress (nrs_iisph_finish first)");
    if (!(f.h > 0.0)) return fail(NRS_E_INVALID, "diffuse particles need interactionRadius > 0");
    for (int a = 0; a < 3; ++a) {
        if (!(f.cellSize[a] >= f.h)) return fail(NRS_E_INVALID, "diffuse particles need cellSize >= interactionRadius on every axis (the 27-cell walk is incomplete otherwise)");
        if (f.gridSize[a] < 4u) return fail(NRS_E_INVALID, "diffuse particles need gridSize >= 4 on every axis (the cells of a row alias through the wrap otherwise)");
        if (f.gridSize[a] & (f.gridSize[a] - 1u)) return fail(NRS_E_INVALID, "diffuse particles need a power-of-two gridSize (the cells of a row alias through the wrap otherwise)");
    }
    return NRS_OK;
}
static inline int diffuse_check_births(uint64_t n, uint32_t maxPer)
{
    if (n * (uint64_t)maxPer > DIFFUSE_MAX_BIRTHS) return fail(NRS_E_INVALID, "diffuse step: particles x max_per_particle above 2^31");
    return NRS_OK;
}
static inline int diffuse_check_upload(const void *pos4, const void *vel4, uint64_t n, uint32_t capacity)
{
    if (n && (!pos4 || !vel4)) return fail(NRS_E_INVALID, "diffuse upload: NULL array");
    if (n > capacity) return fail(NRS_E_INVALID, "diffuse upload: more particles than the configured capacity");
    return NRS_OK;
}

// ---- bytes of a result: D living diffuse particles, N fluid particles of the last step, precision 32 or 64; 0 for anything else ----------
static inline uint64_t diffuse_result_bytes(uint32_t which, uint64_t D, uint64_t N, int precision)
{
    const uint64_t vec4 = precision == 64 ? 32 : 16;
    switch (which) {
    case NRS_DIFFUSE_POS: case NRS_DIFFUSE_VEL: return vec4 * D;
    case NRS_DIFFUSE_KIND: return 4 * D;
    case NRS_DIFFUSE_POTENTIALS: case NRS_DIFFUSE_NORMALS: return vec4 * N;
    case NRS_DIFFUSE_BIRTHS: return 4 * N;
    default: return 0;
    }
}
// what the buffers hold: `configured`, and whether a diffuse step has run since configure / release, over how many fluid particles
struct DiffuseLast {
    bool configured = false, stepped = false;
    uint64_t N = 0;
};
static inline bool diffuse_per_fluid(uint32_t which) { return which == NRS_DIFFUSE_POTENTIALS || which == NRS_DIFFUSE_BIRTHS || which == NRS_DIFFUSE_NORMALS; }
// the refusals first: the caller reads the living count from the device (and waits) only when they pass and the id is per diffuse particle
static inline int diffuse_route_check(const DiffuseLast &last, uint32_t which)
{
    if (which >= DIFFUSE_RESULTS) return fail(NRS_E_INVALID, "which must be one of NRS_DIFFUSE_POS, _VEL, _KIND, _POTENTIALS, _BIRTHS, _NORMALS");
    if (!last.configured) return fail(NRS_E_STATE, "diffuse particles before nrs_diffuse_configure");
    if (diffuse_per_fluid(which) && !last.stepped) return fail(NRS_E_STATE, "no diffuse step yet (or nrs_diffuse_configure / nrs_diffuse_release since)");
    return NRS_OK;
}
static inline int diffuse_route_result(const DiffuseLast &last, uint32_t which, uint64_t alive, int precision, uint64_t *bytes)
{
    NRSCHK(diffuse_route_check(last, which));
    *bytes = diffuse_result_bytes(which, alive, last.N, precision);
    return NRS_OK;
}

// ---- the uniform draws -----------------------------------------------------------------------------------------------------------------
// A counter-based hash of (seed, diffuse steps since configure, fluid slot, draw number), integers only: the finaliser of splitmix64
// applied to the seed and step, then to that word xor (slot << 32 | draw).  A uniform is its top 24 bits times 2^-24.
NRS_DIFF_HD uint64_t diffuse_mix64(uint64_t z)
{
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27; z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}
NRS_DIFF_HD uint64_t diffuse_hash(uint64_t seed, uint64_t step, uint32_t slot, uint32_t draw)
{
    const uint64_t a = diffuse_mix64(seed + 0x9e3779b97f4a7c15ull * (step + 1ull));
    return diffuse_mix64(a ^ (((uint64_t)slot << 32) | (uint64_t)draw));
}
template <typename R> NRS_DIFF_HD R diffuse_uniform(uint64_t seed, uint64_t step, uint32_t slot, uint32_t draw)
{
    return (R)(uint32_t)(diffuse_hash(seed, step, slot, draw) >> 40) * (R)5.9604644775390625e-8; // 2^-24: exact in float and double
}
// draw numbers: 0 the birth count's u; birth k uses 1 + 10 k + (0..7: the four (a, b) pairs, 8: X_h, 9: X_l)
NRS_DIFF_HD uint32_t diffuse_birth_draw(uint32_t k, uint32_t t) { return 1u + DIFFUSE_DRAWS_PER_BIRTH * k + t; }

// ---- a potential and the number of births ------------------------------------------------------------------------------------------------
template <typename R> NRS_DIFF_HD R diffuse_min(R x, R t) { return x < t ? x : t; }
template <typename R> NRS_DIFF_HD R diffuse_clamp(R x, R tmin, R tmax) { return (diffuse_min<R>(x, tmax) - diffuse_min<R>(x, tmin)) / (tmax - tmin); }
template <typename R> NRS_DIFF_HD R diffuse_rate(const DiffuseCfg<R> &c, R ita, R iwc, R ik) { return ik * (c.kTa * ita + c.kWc * iwc); }
template <typename R> NRS_DIFF_HD uint32_t diffuse_births(const DiffuseCfg<R> &c, R rate, R dt, R u)
{
    const R t = rate * dt + u;
    if (t >= (R)c.maxPer) return c.maxPer;
    return t > (R)0 ? (uint32_t)t : 0u; // (floor of a positive number; NaN: none)
}
// 0 spray, 1 foam, 2 bubble by the fluid-neighbour count n
NRS_DIFF_HD uint32_t diffuse_kind(uint32_t n, uint32_t sprayBelow, uint32_t bubbleAbove) { return n < sprayBelow ? 0u : (n > bubbleAbove ? 2u : 1u); }

// ---- small vectors without HIP ---------------------------------------------------------------------------------------------------------------
template <typename R> struct D3 { R x, y, z; };
template <typename R> NRS_DIFF_HD R diffuse_dot(const D3<R> &a, const D3<R> &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
template <typename R> NRS_DIFF_HD float diffuse_length(const D3<R> &a) { return sqrtf((float)diffuse_dot<R>(a, a)); }
template <typename R> NRS_DIFF_HD D3<R> diffuse_cross(const D3<R> &a, const D3<R> &b)
{
    D3<R> c;
    c.x = a.y * b.z - a.z * b.y;
    c.y = a.z * b.x - a.x * b.z;
    c.z = a.x * b.y - a.y * b.x;
    return c;
}

// ---- the birth of one diffuse particle --------------------------------------------------------------------------------------------------------
// xi, vi: the fluid particle of sorted slot `slot`; k: the birth number; rV: particleRadius.  The disc point (a, b): the first of four
// uniform pairs in [-1, 1]^2 inside the unit circle, else the centre.  vhat = vi / length(vi); e1 = normalised vhat x axis, axis the
// coordinate axis of vhat's smallest absolute component (the lowest on a tie), e2 = vhat x e1; |vi| == 0: e1 = x, e2 = y.
//   off = (rV a) e1 + (rV b) e2,   x = (xi + off) + (X_h dt) vi,   v = vi + off (the paper's division by dt is NOT applied),
//   lifetime = min + X_l (max - min)
template <typename R> struct DiffuseBirth { D3<R> x, v; R life; };
template <typename R>
NRS_DIFF_HD DiffuseBirth<R> diffuse_birth(const DiffuseCfg<R> &c, uint64_t step, uint32_t slot, uint32_t k, const D3<R> &xi, const D3<R> &vi, R rV, R dt)
{
    R a = (R)0, b = (R)0;
    for (uint32_t t = 0; t < 4; ++t) {
        const R ua = (R)2 * diffuse_uniform<R>(c.seed, step, slot, diffuse_birth_draw(k, 2 * t)) - (R)1;
        const R ub = (R)2 * diffuse_uniform<R>(c.seed, step, slot, diffuse_birth_draw(k, 2 * t + 1)) - (R)1;
        if (ua * ua + ub * ub < (R)1) { a = ua; b = ub; break; }
    }
    const R xh = diffuse_uniform<R>(c.seed, step, slot, diffuse_birth_draw(k, 8));
    const R xl = diffuse_uniform<R>(c.seed, step, slot, diffuse_birth_draw(k, 9));
    D3<R> e1 = {(R)1, (R)0, (R)0}, e2 = {(R)0, (R)1, (R)0};
    const float vl = diffuse_length<R>(vi);
    if (vl != 0.0f) {
        const R l = (R)vl;
        const D3<R> vh = {vi.x / l, vi.y / l, vi.z / l};
        const R ax = vh.x < (R)0 ? -vh.x : vh.x, ay = vh.y < (R)0 ? -vh.y : vh.y, az = vh.z < (R)0 ? -vh.z : vh.z;
        D3<R> axis = {(R)0, (R)0, (R)0};
        if (ax <= ay && ax <= az) axis.x = (R)1;
        else if (ay <= az) axis.y = (R)1;
        else axis.z = (R)1;
        const D3<R> t1 = diffuse_cross<R>(vh, axis);
        const R tl = (R)diffuse_length<R>(t1);
        e1.x = t1.x / tl; e1.y = t1.y / tl; e1.z = t1.z / tl;
        e2 = diffuse_cross<R>(vh, e1);
    }
    const R ra = rV * a, rb = rV * b, s = xh * dt;
    const D3<R> off = {ra * e1.x + rb * e2.x, ra * e1.y + rb * e2.y, ra * e1.z + rb * e2.z};
    DiffuseBirth<R> o;
    o.x.x = (xi.x + off.x) + s * vi.x; o.x.y = (xi.y + off.y) + s * vi.y; o.x.z = (xi.z + off.z) + s * vi.z;
    o.v.x = vi.x + off.x; o.v.y = vi.y + off.y; o.v.z = vi.z + off.z;
    o.life = c.lifeMin + xl * (c.lifeMax - c.lifeMin);
    return o;
}

// ---- the advection of one diffuse particle ----------------------------------------------------------------------------------------------------
// x, v, life: its state; vt, n: the Shepard velocity and the fluid-neighbour count of sample_walk at x (vt = 0 where n = 0); g: gravity;
// lo, hi: the grid box [worldOrigin, worldOrigin + gridSize cellSize).
//   spray:  v += dt g,                                       x += dt v
//   foam:   v = vt,                                          x += dt vt,   life -= dt
//   bubble: v = (v + dt ((-k_buoyancy) g)) + k_drag (vt - v), x += dt v
// dead: life <= 0, a non-finite coordinate, or a coordinate outside the box
template <typename R> struct DiffuseState { D3<R> x, v; R life; uint32_t kind; bool alive; };
template <typename R> NRS_DIFF_HD bool diffuse_inside(R x, R lo, R hi) { return x >= lo && x < hi && x - x == (R)0; }
template <typename R>
NRS_DIFF_HD DiffuseState<R> diffuse_advect(const DiffuseCfg<R> &c, D3<R> x, D3<R> v, R life, const D3<R> &vt, uint32_t n, const D3<R> &g, R dt,
                                           const D3<R> &lo, const D3<R> &hi)
{
    DiffuseState<R> o;
    o.kind = diffuse_kind(n, c.sprayBelow, c.bubbleAbove);
    if (o.kind == 0u) {
        v.x = v.x + dt * g.x; v.y = v.y + dt * g.y; v.z = v.z + dt * g.z;
    } else if (o.kind == 1u) {
        v = vt;
        life = life - dt;
    } else {
        const R nb = -c.kBuoyancy;
        v.x = (v.x + dt * (nb * g.x)) + c.kDrag * (vt.x - v.x);
        v.y = (v.y + dt * (nb * g.y)) + c.kDrag * (vt.y - v.y);
        v.z = (v.z + dt * (nb * g.z)) + c.kDrag * (vt.z - v.z);
    }
    x.x = x.x + dt * v.x; x.y = x.y + dt * v.y; x.z = x.z + dt * v.z;
    o.x = x; o.v = v; o.life = life;
    o.alive = life > (R)0 && diffuse_inside<R>(x.x, lo.x, hi.x) && diffuse_inside<R>(x.y, lo.y, hi.y) && diffuse_inside<R>(x.z, lo.z, hi.z);
    return o;
}

} // namespace nrs
