// nrs_host_track.h — the host decisions of particle tracking (include/nereus_hip.h "particle identity and attributes"; DESIGN.md
// "Particle identity and attributes"), written once: which flags, result ids, uploads, ranges and coefficients are accepted and the
// refusal texts; the id accounting (fresh ranges, next_id after an id upload, exhaustion); the saturating birth stamp; which slots an
// upload or a count change treats as new; how many bytes a result takes.  No HIP: the owner of the device buffers (TrackSystem,
// nrs_track.h), the context (nrs_ctx_impl.h) and a plain host program (tests/host_track_main.cpp) call the same routines.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "nrs_error.h"

namespace nrs {

constexpr uint32_t TRACK_KNOWN_FLAGS = NRS_TRACK_ATTR;
constexpr uint64_t TRACK_LAST_ID = 0xfffffffeull;   // the largest id; NRS_TRACK_NONE is never one
constexpr uint64_t TRACK_MAX_LOCATE = 1ull << 27;
constexpr int TRACK_EMIT_VALUES = NRS_MAX_EMITTERS + 1; // [0]: slot -1 (nrs_emit_block, appended uploads, count growth), [1 + s]: emitter s

// ---- enable, and the contexts that cannot track ------------------------------------------------------------------------------------------
static inline int track_check_flags(uint32_t flags)
{
    if (flags & ~TRACK_KNOWN_FLAGS) return fail(NRS_E_INVALID, "particle tracking: flags has unknown bits");
    return NRS_OK;
}
static inline int track_refuse_slab() { return fail(NRS_E_INVALID, "particle tracking on a slab context (its arrays hold halo copies)"); }
static inline int track_refuse_slab_configure() { return fail(NRS_E_INVALID, "nrs_slab_configure on a context that tracks its particles"); }

// ---- the state a call is refused in --------------------------------------------------------------------------------------------------------
// needAttr: the call is about the attribute record; settled: it reads or moves the tracked arrays of a completed state (result, pointer,
// locate, diffuse)
struct TrackFacts {
    bool on;
    uint32_t flags;
    bool midStep, iisphInProgress;
};
static inline int track_refusal(const TrackFacts &f, bool needAttr, bool settled)
{
    if (!f.on) return fail(NRS_E_STATE, "particle tracking before nrs_track_enable");
    if (needAttr && !(f.flags & NRS_TRACK_ATTR)) return fail(NRS_E_STATE, "particle tracking: the context was enabled without NRS_TRACK_ATTR, there is no attribute record");
    if (settled && f.midStep) return fail(NRS_E_STATE, "particle tracking while the state is mid-update after nrs_step_partial");
    if (settled && f.iisphInProgress) return fail(NRS_E_STATE, "particle tracking while a host-driven IISPH step is in progress (nrs_iisph_finish first)");
    return NRS_OK;
}

// ---- ids and births --------------------------------------------------------------------------------------------------------------------------
// birth = the completed-step counter at the moment the particle entered, saturating
static inline uint32_t track_birth(uint64_t stepsDone) { return stepsDone > 0xffffffffull ? 0xffffffffu : (uint32_t)stepsDone; }
// `count` fresh consecutive ids would start at `next`: refused, with nothing changed, when the last of them passes TRACK_LAST_ID
static inline int track_ids_fit(uint64_t next, uint64_t count)
{
    if (count && (next > TRACK_LAST_ID || count - 1 > TRACK_LAST_ID - next)) return fail(NRS_E_CAPACITY, "particle ids exhausted; nrs_track_enable renumbers");
    return NRS_OK;
}
struct TrackIds {
    uint64_t next = 0;
    int reserve(uint64_t count, uint32_t *first)
    {
        NRSCHK(track_ids_fit(next, count));
        *first = (uint32_t)next; // (count == 0: not used)
        next += count;
        return NRS_OK;
    }
};
// next_id after an upload of ids: the larger of itself and one plus the largest uploaded id; NRS_TRACK_NONE is refused before anything is stored
static inline int track_ids_uploaded(const uint32_t *src, uint64_t count, uint64_t next, uint64_t *nextOut)
{
    uint64_t m = next;
    for (uint64_t i = 0; i < count; ++i) {
        if (src[i] == NRS_TRACK_NONE) return fail(NRS_E_INVALID, "particle tracking: NRS_TRACK_NONE is not an id");
        if ((uint64_t)src[i] + 1 > m) m = (uint64_t)src[i] + 1;
    }
    *nextOut = m;
    return NRS_OK;
}

// ---- which slots are new ------------------------------------------------------------------------------------------------------------------------
// nrs_upload_particles(first, count) on n particles: slots below n are the same particle, moved; [n, first + count) are new.
// nrs_set_num_particles(nn): shrinking drops the tail, growing makes [n, nn) new.
struct TrackFresh { uint64_t first, count; };
static inline TrackFresh track_fresh_after_upload(uint64_t n, uint64_t first, uint64_t count)
{
    const uint64_t end = first + count;
    return end > n ? TrackFresh{n, end - n} : TrackFresh{n, 0};
}
static inline TrackFresh track_fresh_after_set_n(uint64_t n, uint64_t nn) { return nn > n ? TrackFresh{n, nn - n} : TrackFresh{nn, 0}; }

// ---- nrs_track_upload ---------------------------------------------------------------------------------------------------------------------------
static inline int track_check_upload(uint32_t which, uint32_t flags, const void *src, uint64_t first, uint64_t count, uint64_t n)
{
    if (which != NRS_TRACK_ID && which != NRS_TRACK_BIRTH && which != NRS_TRACK_ATTRIBUTE)
        return fail(NRS_E_INVALID, "particle tracking: an upload takes NRS_TRACK_ID, NRS_TRACK_BIRTH or NRS_TRACK_ATTRIBUTE");
    if (which == NRS_TRACK_ATTRIBUTE && !(flags & NRS_TRACK_ATTR))
        return fail(NRS_E_STATE, "particle tracking: the context was enabled without NRS_TRACK_ATTR, there is no attribute record");
    if (first > n || count > n - first) return fail(NRS_E_INVALID, "particle tracking: an upload must lie inside [0, n)");
    if (count && !src) return fail(NRS_E_INVALID, "particle tracking: src is NULL");
    return NRS_OK;
}

// ---- results ------------------------------------------------------------------------------------------------------------------------------------
// bytes of a result: n living particles, `located` entries of the last nrs_track_locate
static inline uint64_t track_result_bytes(uint32_t which, uint64_t n, uint64_t located, int precision)
{
    switch (which) {
    case NRS_TRACK_ID: case NRS_TRACK_BIRTH: return 4 * n;
    case NRS_TRACK_ATTRIBUTE: return (precision == 64 ? 32 : 16) * n;
    case NRS_TRACK_SLOT_OF: return 4 * located;
    default: return 0;
    }
}
static inline int track_route_result(uint32_t which, uint32_t flags, bool haveLocate, uint64_t n, uint64_t located, int precision, uint64_t *bytes)
{
    if (which != NRS_TRACK_ID && which != NRS_TRACK_BIRTH && which != NRS_TRACK_ATTRIBUTE && which != NRS_TRACK_SLOT_OF)
        return fail(NRS_E_INVALID, "particle tracking: which must be NRS_TRACK_ID, _BIRTH, _ATTRIBUTE or _SLOT_OF");
    if (which == NRS_TRACK_ATTRIBUTE && !(flags & NRS_TRACK_ATTR))
        return fail(NRS_E_STATE, "particle tracking: the context was enabled without NRS_TRACK_ATTR, there is no attribute record");
    if (which == NRS_TRACK_SLOT_OF && !haveLocate) return fail(NRS_E_STATE, "particle tracking: no nrs_track_locate since nrs_track_enable");
    *bytes = track_result_bytes(which, n, located, precision);
    return NRS_OK;
}

// ---- the emit values, locate, diffuse -----------------------------------------------------------------------------------------------------------
static inline int track_check_emit_value(int32_t slot, const double *a)
{
    if (slot < -1 || slot >= (int32_t)NRS_MAX_EMITTERS) return fail(NRS_E_INVALID, "particle tracking: an emit value's slot is -1 or below NRS_MAX_EMITTERS (16)");
    if (!a) return fail(NRS_E_INVALID, "particle tracking: the emit value is NULL");
    return NRS_OK;
}
static inline int track_check_locate(uint64_t firstId, uint64_t count)
{
    (void)firstId; // (any start: ids that do not exist are simply absent)
    if (count > TRACK_MAX_LOCATE) return fail(NRS_E_INVALID, "particle tracking: nrs_track_locate takes at most 2^27 ids");
    return NRS_OK;
}
static inline int track_check_diffuse(const double *kappa, double dt)
{
    if (!kappa) return fail(NRS_E_INVALID, "particle tracking: kappa is NULL");
    for (int c = 0; c < 4; ++c)
        if (!std::isfinite(kappa[c]) || kappa[c] < 0.0) return fail(NRS_E_INVALID, "particle tracking: kappa must be finite and >= 0");
    if (!std::isfinite(dt) || dt < 0.0) return fail(NRS_E_INVALID, "particle tracking: dt must be finite and >= 0 (0: the context's timestep)");
    return NRS_OK;
}

} // namespace nrs
