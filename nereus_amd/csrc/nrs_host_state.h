// nrs_host_state.h — the state of the particle arrays and of the keys prepared for the next step, and what the sort stage makes of it.
// No HIP: bools and counts in, a state or a choice out.  The context (nrs_ctx_impl.h) holds one ArrayTracker; the device pointers
// the fields speak about (hashNext / indexNext, hashCur / indexCur, packKeys / packVals) are SortStage's (nrs_sort.h).  The context
// launches, then names what happened.
#pragma once
#include <cstdint>

#include "nrs_error.h"

namespace nrs {

// coherent re-sort (nrs_kernels_resort.h): when a step takes it
constexpr uint64_t RESORT_MIN_PARTICLES = 32768; // below this the full sort is launch-bound either way
constexpr uint32_t RESORT_MAX_MOVER_PCT = 50;    // more movers than this share of N: full radix sort (measured break-even,
                                                 // DESIGN.md §4)
static inline bool few_movers(uint64_t M, uint64_t N) { return M * 100ull <= N * (uint64_t)RESORT_MAX_MOVER_PCT; }
// big, mostly empty cell table: a step undoes only the cells it touched (k_clear_cells, or the split's ride-along reset)
static inline bool sparse_cell_table(uint64_t numCells, uint64_t n) { return numCells > 8ull * n; }

// The fields are not independent: they encode ONE of the states below (DESIGN.md §5 has the table of the states, §4 "Array state,
// step plan and sort choice" that of the transitions).  Every public entry point calls validate() first, so a sequence of calls
// that would leave them inconsistent returns NRS_E_STATE instead of handing a wrong count or a stale table to a kernel (the GPU
// memory fault of round 1 was exactly that: a merge sized with a mover count that had been reset before it was read).
struct ArrayFields {
    bool hashReady = false;       // the fused force kernel already wrote the next step's keys/values (hashNext / indexNext)
    bool rsPending = false;       // movers/stayers of the keys in hashNext have been split; the count is on its way
    bool rsCountKnown = false;    // the mover count of the pending split is already on the host (slab runs)
    uint32_t rsKnownCount = 0;
    bool slotOrderValid = false;  // posA/velA are in the slot order of hashCur (a full fused step was the last thing that happened)
    bool classifiedValid = false; // the force kernel of the last step already wrote stream flags / counts / dead marks for these cuts ...
    uint32_t classifiedN = 0;     // ... of this many slots
    bool holesPending = false;    // posA/velA[0, physN) contain dead slots (keys in hashNext tell which); n counts live ones
    uint32_t physN = 0;           // physical extent of the arrays while holesPending
    bool packedHashValid = false; // packKeys hold the keys of the particles that stayed, for the current grid
};
// what array_state() reads besides the fields
struct ArrayFacts {
    uint64_t n, cap, nOwned;
    bool slabOn, inplace;                        // a slab run; the last pack partitioned in place (SlabHost::inplace())
    bool hashNext, indexNext, hashCur, rsMovers; // the pointer / buffer of that name is there
};
enum ArrayState {
    AS_FRESH,        // arrays compact, any order; the next step hashes and sorts from scratch
    AS_KEYS_READY,   // + hashNext/indexNext hold the next step's keys/values (fused kernel, or slab pack/unpack)
    AS_SPLIT_QUEUED, // + their movers/stayers split is queued (coherent re-sort); the count is pending or known
    AS_SLOT_ORDER,   // slab run after a fused step: arrays in the slot order of hashCur, keys per slot, to be re-partitioned
    AS_HOLES,        // slab in-place partition: arrays [0, physN) with dead slots, split queued, count known
    AS_INVALID
};
static inline ArrayState array_state(const ArrayFields &f, const ArrayFacts &a)
{
    if (a.n > a.cap || (a.slabOn && a.nOwned > a.n)) return AS_INVALID;
    if (!a.slabOn && (f.holesPending || f.classifiedValid)) return AS_INVALID;
    if (f.hashReady && (!a.hashNext || !a.indexNext)) return AS_INVALID;
    if (f.rsPending && (!f.hashReady || !a.rsMovers)) return AS_INVALID;
    if (f.rsCountKnown && !f.rsPending) return AS_INVALID;
    if (f.classifiedValid && (!f.slotOrderValid || !a.hashCur || !a.hashNext)) return AS_INVALID;
    if (f.slotOrderValid && (!a.hashCur || !a.hashNext)) return AS_INVALID;
    if (f.holesPending) {
        if (!(a.inplace && f.hashReady && f.rsPending && f.rsCountKnown) || f.physN < a.n || f.physN > a.cap || f.rsKnownCount > f.physN)
            return AS_INVALID;
        return AS_HOLES;
    }
    if (f.rsCountKnown && f.rsKnownCount > a.n) return AS_INVALID;
    if (f.rsPending) return AS_SPLIT_QUEUED;
    if (f.hashReady) return AS_KEYS_READY;
    if (f.slotOrderValid) return AS_SLOT_ORDER;
    return AS_FRESH;
}

// The fields, readable by everybody and written by the transitions below alone (round 3: they used to be set one by one at ~30
// places, which is how a count could be reset before it was read); array_state() reads the result back as ONE state.
struct ArrayTracker {
    const ArrayFields &fields() const { return f; }
    void drop_prepared_keys() { f.hashReady = false; f.rsPending = false; f.rsCountKnown = false; }   // the keys were consumed, or are void
    void to_fresh() { drop_prepared_keys(); f.slotOrderValid = false; f.classifiedValid = false; }   // -> AS_FRESH: compact arrays, any order
    void keys_ready() { f.hashReady = true; }                                                        // -> AS_KEYS_READY (Ctx::keys_ready: SortStage::keys_written first)
    void split_queued() { f.rsPending = true; }                                                      // -> AS_SPLIT_QUEUED, count still on the device
    void split_queued_known(uint32_t movers) { f.rsPending = true; f.rsCountKnown = true; f.rsKnownCount = movers; } // ..., count on the host
    void to_holes(uint32_t extent, uint32_t movers)                                                  // -> AS_HOLES (in-place slab partition)
    {
        f.holesPending = true; f.physN = extent; f.packedHashValid = true; f.hashReady = true;
        split_queued_known(movers);
    }
    void holes_consumed() { f.holesPending = false; }  // the reorder's gather reads only live slots: the B arrays are compact
    void holes_compacted() { f.holesPending = false; drop_prepared_keys(); f.packedHashValid = false; } // compact_holes: and the prepared re-sort is forgotten
    void grid_changed() { to_fresh(); f.packedHashValid = false; } // every key computed for the old grid is void
    void classification_dropped() { f.classifiedValid = false; }   // a fused launch without a classification is about to overwrite the keys
    void classified(uint32_t N) { f.classifiedValid = true; f.classifiedN = N; } // the fused launch classifies N slots for the current cuts
    void cuts_changed() { f.classifiedValid = false; f.slotOrderValid = false; } // classified (dead keys marked) for other cuts: partition the slow way once
    void pack_hashed(bool hashed) { f.packedHashValid = hashed; }  // a compacting pack: k_slab_scatter hashed the particles that stay, if any
    void arrivals_appended(bool inplace, uint32_t arrivals)        // pack + unpack have written the keys/values of every local particle
    {
        f.hashReady = f.packedHashValid;
        if (inplace) { f.physN += arrivals; f.rsKnownCount += arrivals; } // every arrival is a mover (k_slab_append put it behind the cell changers)
    }
    void step_ended(bool fused) { f.slotOrderValid = fused; }      // fused: A holds the new state in the slot order of hashCur

private:
    ArrayFields f;
};

// ---- the sort stage's choice (stage_prefix reads it and launches) -------------------------------------------------------------------
struct ResortStats { // nrs_resort_stats, NRS_STAT_MOVERS
    uint64_t steps = 0, fallbacks = 0; // steps that had a split queued; of them, those that sorted in full all the same
    double lastMovers = -1.0;          // mover count of the last coherent re-sort
};
struct SortPrefix {
    bool compactFirst; // arrays with holes that the merge path cannot consume: compact_holes() first, then hash and sort from scratch
    bool useKeys;      // the keys / values of this step are the prepared ones (no hash launch)
    bool resort;       // ... and their queued split is used: choose_sort() with the mover count
    bool countKnown;   // ... which the host already has (slab runs): knownCount
    uint32_t knownCount;
};
// In-place slab partition: only the merge path can consume arrays with holes; a queued split given up for that is a step and a fallback.
static inline SortPrefix choose_sort_prefix(const ArrayFields &f, int stop, uint64_t n, ResortStats &rs)
{
    const bool sorts = stop != NRS_STAGE_HASH && stop != NRS_STAGE_SORT;
    const bool split = f.hashReady && f.rsPending && f.rsCountKnown;
    SortPrefix c = {false, f.hashReady, f.hashReady && f.rsPending && sorts, f.rsCountKnown, f.rsKnownCount};
    if (f.holesPending && !(split && sorts && few_movers(f.rsKnownCount, n))) {
        if (split) { ++rs.steps; ++rs.fallbacks; }
        c.compactFirst = true; // also drops the prepared keys
        c.useKeys = false; c.resort = false; c.countKnown = false;
    }
    return c;
}
enum class SortKind {
    MERGE_STAYERS, // no mover: the stayers are the sorted sequence
    MERGE_MOVERS,  // mover sort + merge with the stayers
    FULL_SORT      // too many movers: the full radix sort, counted as a fallback
};
// The split of these keys into movers / stayers was queued behind the kernel that wrote them; its mover count M sizes the mover sort
// and the merge (nrs_kernels_resort.h).
static inline int choose_sort(uint64_t M, uint64_t N, ResortStats &rs, SortKind &kind)
{
    ++rs.steps;
    rs.lastMovers = (double)M;
    kind = SortKind::FULL_SORT;
    if (M > N) return fail(NRS_E_STATE, "coherent re-sort: mover count exceeds the particle count (stale count)");
    if (few_movers(M, N)) kind = M == 0 ? SortKind::MERGE_STAYERS : SortKind::MERGE_MOVERS;
    else ++rs.fallbacks;
    return NRS_OK;
}

} // namespace nrs
