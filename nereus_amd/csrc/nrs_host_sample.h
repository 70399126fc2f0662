// nrs_host_sample.h — the host decisions of the field sampler (include/nereus_hip.h "field sampling"; DESIGN.md "Field sampling"): which
// flags and lattices are accepted, how many nodes a lattice has, how many bytes a result takes, when a context refuses to
// sample, when the sampler's particle grid has to be rebuilt, and which result of the last call a field id means.  No HIP: plain facts
// in, a size or a refusal out.  The owner of the device buffers (FieldSampler, nrs_field_sampler.h) and its holder (nrs_readers.h) launch, then name
// what happened.
#pragma once
#include <cmath>
#include <cstdint>

#include "nrs_error.h"

namespace nrs {

constexpr uint32_t SAMPLE_OUTPUTS = NRS_FIELD_DENSITY | NRS_FIELD_GRADIENT | NRS_FIELD_VELOCITY | NRS_FIELD_COUNT;
constexpr uint32_t SAMPLE_KNOWN = SAMPLE_OUTPUTS | NRS_FIELD_WALLS;
constexpr uint64_t SAMPLE_MAX_QUERIES = 1ull << 31; // a query index is a 32-bit launch index

// ---- what a call may ask for -------------------------------------------------------------------------------------------------------
static inline int sample_check_fields(uint32_t fields)
{
    if (fields & ~SAMPLE_KNOWN) return fail(NRS_E_INVALID, "fields has unknown bits");
    if (!(fields & SAMPLE_OUTPUTS)) return fail(NRS_E_INVALID, "fields names no output (NRS_FIELD_DENSITY, _GRADIENT, _VELOCITY, _COUNT)");
    return NRS_OK;
}
static inline int sample_check_points(const void *points4, uint64_t m)
{
    if (m && !points4) return fail(NRS_E_INVALID, "points4 is NULL");
    if (m > SAMPLE_MAX_QUERIES) return fail(NRS_E_INVALID, "more than 2^31 points");
    return NRS_OK;
}
// nodes of a lattice; 0 for a dim of 0 (the factors are 32-bit: the first product cannot wrap, the second is formed in two steps)
static inline uint64_t lattice_nodes(const uint32_t dims[3])
{
    const uint64_t xy = (uint64_t)dims[0] * dims[1];
    if (!xy || !dims[2]) return 0;
    if (xy > SAMPLE_MAX_QUERIES) return UINT64_MAX;
    return xy * dims[2]; // <= 2^31 * (2^32 - 1)
}
static inline int sample_check_lattice(const nrs_lattice *L, uint64_t *nodes)
{
    if (!L) return fail(NRS_E_INVALID, "lattice is NULL");
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(L->origin[a])) return fail(NRS_E_INVALID, "lattice origin is not finite");
        if (!std::isfinite(L->spacing[a]) || !(L->spacing[a] > 0.0)) return fail(NRS_E_INVALID, "lattice spacing must be finite and > 0");
        if (!L->dims[a]) return fail(NRS_E_INVALID, "lattice dim of 0");
    }
    const uint64_t n = lattice_nodes(L->dims);
    if (n > SAMPLE_MAX_QUERIES) return fail(NRS_E_INVALID, "lattice has more than 2^31 nodes");
    if (nodes) *nodes = n;
    return NRS_OK;
}
// a validated nrs_lattice as the kernels and the host routines of the sampler, the surface extraction and nrs_emit_block get it
struct Lattice {
    double origin[3], spacing[3];
    uint32_t dims[3];
};
static inline Lattice lattice_from(const nrs_lattice &l)
{
    Lattice L;
    for (int a = 0; a < 3; ++a) { L.origin[a] = l.origin[a]; L.spacing[a] = l.spacing[a]; L.dims[a] = l.dims[a]; }
    return L;
}

// ---- bytes of a result: `field` is ONE output flag, m the queries of the call, precision 32 or 64; 0 for anything else ------------------
static inline uint64_t sample_result_bytes(uint32_t field, uint64_t m, int precision)
{
    const uint64_t real = precision == 64 ? 8 : 4;
    switch (field) {
    case NRS_FIELD_DENSITY: return real * m;
    case NRS_FIELD_GRADIENT: case NRS_FIELD_VELOCITY: return 4 * real * m;
    case NRS_FIELD_COUNT: return 4 * m;
    default: return 0;
    }
}

// ---- when a context refuses to sample ------------------------------------------------------------------------------------------------
struct SampleFacts {
    bool midStep;         // state is mid-update after nrs_step_partial
    bool iisphInProgress; // between nrs_iisph_predict and nrs_iisph_finish
    bool slab;            // the context has a slab decomposition
    uint32_t gridSize[3];
    double cellSize[3], h;
};
static inline int sample_refusal(const SampleFacts &f)
{
    if (f.slab) return fail(NRS_E_INVALID, "field sampling on a slab context (its arrays hold halo copies)");
    if (f.midStep) return fail(NRS_E_STATE, "field sampling while the state is mid-update after nrs_step_partial");
    if (f.iisphInProgress) return fail(NRS_E_STATE, "field sampling while a host-driven IISPH step is in progress (nrs_iisph_finish first)");
    if (!(f.h > 0.0)) return fail(NRS_E_INVALID, "field sampling needs interactionRadius > 0");
    for (int a = 0; a < 3; ++a) {
        if (!(f.cellSize[a] >= f.h)) return fail(NRS_E_INVALID, "field sampling needs cellSize >= interactionRadius on every axis (the 27-cell walk is incomplete otherwise)");
        if (f.gridSize[a] < 4u) return fail(NRS_E_INVALID, "field sampling needs gridSize >= 4 on every axis (the cells of a row alias through the wrap otherwise)");
        if (f.gridSize[a] & (f.gridSize[a] - 1u)) return fail(NRS_E_INVALID, "field sampling needs a power-of-two gridSize (the cells of a row alias through the wrap otherwise)");
    }
    return NRS_OK;
}

// ---- the cache rule: the sampler's sorted particles and cell table describe one particle state on one grid ----------------------------
// The context counts what changes them: completed steps, uploads / nrs_set_num_particles, grid changes, boundary changes (a new set, a
// body assignment: the boundary tables may have been rebuilt on another grid, and moving walls move with the steps).
struct SampleKey {
    uint64_t stepsDone, particleGen, gridGen, boundaryGen;
    bool operator==(const SampleKey &o) const
    {
        return stepsDone == o.stepsDone && particleGen == o.particleGen && gridGen == o.gridGen && boundaryGen == o.boundaryGen;
    }
};
struct SampleCache {
    bool valid = false;
    SampleKey key = {0, 0, 0, 0};
    uint64_t builds = 0; // nrs_sample_builds
    bool needs_build(const SampleKey &now) const { return !valid || !(key == now); }
    void built(const SampleKey &now) { valid = true; key = now; ++builds; }
    void dropped() { valid = false; } // nrs_sample_release: the buffers are gone (the count of builds stays)
};

// ---- which result a field id means: the last call's, or a refusal ---------------------------------------------------------------------
struct SampleLast {
    bool any = false;    // a sample call has completed since nrs_create / nrs_sample_release
    uint32_t fields = 0; // its flags
    uint64_t m = 0;      // its queries
};
static inline int sample_route_result(const SampleLast &last, uint32_t field, int precision, uint64_t *bytes)
{
    if (field != NRS_FIELD_DENSITY && field != NRS_FIELD_GRADIENT && field != NRS_FIELD_VELOCITY && field != NRS_FIELD_COUNT)
        return fail(NRS_E_INVALID, "field must be one of NRS_FIELD_DENSITY, _GRADIENT, _VELOCITY, _COUNT");
    if (!last.any) return fail(NRS_E_STATE, "no sample call yet (or nrs_sample_release since)");
    if (!(last.fields & field)) return fail(NRS_E_STATE, "the last sample call did not compute this field");
    *bytes = sample_result_bytes(field, last.m, precision);
    return NRS_OK;
}

} // namespace nrs
