// nrs_sort.h — the sort stage of a context: the (hash, index) key pairs and which of each pair is current, prepared or a pack target,
// the radix sort's workspace, every buffer of the coherent re-sort (nrs_kernels_resort.h has the scheme) and of its dead-slot twin, the
// pinned mover-count word, the re-sort's statistics.  None of it depends on the precision, the kernel set or SURF: SortStage is a plain
// struct, the context (nrs_ctx_impl.h) holds one, reads it through the views below and drives it through the named operations.
// nrs_sort.hip defines them and launches the three kernels that need no precision (nrs_kernels_sort.h: scan of the tile counts, split,
// count of dead slots); it is the one translation unit of libnereus_hip.so that includes the radix-sort library; this header does not.
#pragma once
#include "nrs_ctx_base.h"
#include "nrs_host_state.h"

namespace nrs {

constexpr int RESORT_GROUP = 1024; // tiles per scan workgroup (RESORT_MIN_PARTICLES, RESORT_MAX_MOVER_PCT: nrs_host_state.h)
struct ResortScan { // one scanned array: counts in, offsets (local to the group) + group totals/prefixes out
    uint32_t *tile, *tileOffset, *groupTotal, *groupPrefix, *total;
};
struct ResortOffsets { const uint32_t *tileOffset, *groupPrefix; }; // what a consumer of a scan reads: groupPrefix[t / RESORT_GROUP] + tileOffset[t]

// ---- plain (uint32 key, uint32 value) pairs: the boundary sorts (nrs_boundary_tables.h, nrs_boundary.hip) ----------------------------
// The library's default configuration at every key width (the fluid's sort below picks wider digits for 25-30 bits: two rules, on
// purpose).  tmp == nullptr: only the workspace size, into `bytes`.  On return key / val are the buffers the sorted pairs ended in.
struct PairBuffers { uint32_t *key, *keyAlt, *val, *valAlt; };
hipError_t sort_pairs_plain(void *tmp, size_t &bytes, PairBuffers &p, size_t n, unsigned bits, hipStream_t stream);

struct KeyPair { uint32_t *hash, *index; };
// which keys k_resort_split compares the prepared ones with
enum class SplitFrom {
    SORTED,       // this step's sorted keys
    SORTED_HOLES, // ... of an in-place slab partition: a prepared key 0xffffffff is a dead slot, counted by the dead twin
    PACKED        // the compacted old keys a compacting slab partition left (prev_packed())
};

struct SortStage {
    // the pairs, the workspace for `cap` particles (the largest of three pair-sort and three mover-sort configurations and the merge)
    // and, with `resort`, the buffers of the coherent re-sort; every later launch goes to `stream`
    int init(uint64_t cap, bool resort, hipStream_t stream);

    // ---- views -----------------------------------------------------------------------------------------------------------------------
    uint32_t *hash() const { return hashCur; }   // sorted keys / values after the sort stage (null before the first one)
    uint32_t *index() const { return indexCur; }
    KeyPair prepared() const { return KeyPair{hashNext, indexNext}; } // the next step's keys / values, once written (st: hashReady)
    KeyPair next_keys() const { return KeyPair{other(hashA, hashB, hashCur), other(indexA, indexB, indexCur)}; } // where a step's last launch writes them
    KeyPair pack_keys() const { return KeyPair{packKeys, packVals}; } // where slab_pack / slab_unpack write them
    bool has_resort() const { return rsMovers.p != nullptr; }
    const ResortStats &stats() const { return rs; }
    uint32_t *tile_movers() const { return rsTileMovers.as<uint32_t>(); } // per 256-slot tile: cell changers, counted by whoever writes the keys
    uint32_t *tile_dead() const { return rsTileDead.as<uint32_t>(); }     // ... and dead slots (slab runs)
    uint32_t *prev_packed() const { return rsPrevPacked.as<uint32_t>(); } // compacting slab partition: the old keys of the particles that stay
    uint64_t *movers() const { return rsMovers.as<uint64_t>(); }          // in-place slab partition: k_slab_append adds the arrivals
    const uint32_t *scan_scalars() const { return rsScalars.as<uint32_t>(); } // 16 bytes: [1] cell changers, [2] dead slots of the last scan
    ResortOffsets offsets_dead() const { return ResortOffsets{rsTileDeadOffset.as<uint32_t>(), rsGroupDeadPrefix.as<uint32_t>()}; }

    // ---- which buffer of each pair is what ---------------------------------------------------------------------------------------------
    void take_fresh() { hashCur = hashA.as<uint32_t>(); indexCur = indexA.as<uint32_t>(); } // k_hash writes this step's keys into hash() / index()
    void take_prepared() { hashCur = hashNext; indexCur = indexNext; }                      // this step's keys are the prepared ones
    void keys_written() { const KeyPair k = next_keys(); hashNext = k.hash; indexNext = k.index; } // a step's last launch wrote next_keys()
    // slab_pack: in place the prepared keys / slot numbers stay where they are; the compacting form hashes into next_keys()
    KeyPair pack_targets(bool inplace)
    {
        const KeyPair k = inplace ? prepared() : next_keys();
        packKeys = k.hash; packVals = k.index;
        return k;
    }
    void pack_targets_empty() { packKeys = hashA.as<uint32_t>(); packVals = indexA.as<uint32_t>(); } // a compacting pack of no particle
    void pack_wrote_every_key() { hashNext = packKeys; indexNext = packVals; } // pack + unpack: the keys / values of every local particle

    // ---- the sort ----------------------------------------------------------------------------------------------------------------------
    SortPrefix choose_prefix(const ArrayFields &f, int stop, uint64_t n) { return choose_sort_prefix(f, stop, n, rs); }
    // Sorts the N keys taken.  With c.resort the queued split is used: its mover count (waited for unless the host has it) goes to
    // choose_sort(); few movers: mover sort + merge, or the stayers alone, *merged gets the u64 pairs for k_reorder_merged and hash() /
    // index() the buffers it writes the plain arrays to.  Otherwise the full pair sort, *merged null, hash() / index() where it ended.
    int sort_keys(const SortPrefix &c, uint32_t N, unsigned bits, const uint64_t **merged);

    // ---- tile counts, scan, split ------------------------------------------------------------------------------------------------------
    int clean_tile_counts();                      // zero tile_movers() / tile_dead() if they hold counts no scan has consumed
    void tile_counts_written() { rsTilesDirty = true; } // a launch counts into them that a scan may never consume
    // exclusive scan of any tile counts (k_resort_scan_tiles), nothing to the host: the wall list's
    int scan_tiles(const ResortScan &a, uint32_t *done, uint32_t nTiles) const;
    // the scan of tile_movers(), with the dead twin or not; the mover total also goes to the pinned word sort_keys() waits for
    int scan_movers(uint32_t nTiles, bool withDead);
    // the dead slots among the N prepared keys, counted per tile and scanned (offsets_dead()): what k_holes_compact needs
    int scan_holes(uint32_t N);
    // stable split of the N prepared keys into movers / stayers behind scan_movers(); clearCells (cellStart, or null): also undo the cell table
    int split(SplitFrom from, uint32_t N, uint32_t *clearCells);

private:
    hipStream_t stream = nullptr;
    DevBuf hashA, hashB, indexA, indexB, sortTmp;
    uint32_t *hashCur = nullptr, *indexCur = nullptr;
    uint32_t *hashNext = nullptr, *indexNext = nullptr;
    uint32_t *packKeys = nullptr, *packVals = nullptr;
    // the buffer of the pair (a, b) that cur is not: where a sort or the next step's keys / values go
    static uint32_t *other(const DevBuf &a, const DevBuf &b, const uint32_t *cur) { return cur == a.as<uint32_t>() ? b.as<uint32_t>() : a.as<uint32_t>(); }
    DevBuf rsMovers, rsMoversAlt, rsStayers, rsMerged, rsTileMovers, rsTileOffset, rsGroupTotal, rsGroupPrefix, rsScalars, rsPrevPacked;
    // slab runs, in-place partition: the owned particles are not compacted; dead slots carry the key 0xffffffff
    DevBuf rsTileDead, rsTileDeadOffset, rsGroupDeadTotal, rsGroupDeadPrefix;
    PinnedBuf<uint64_t> rsHostTotal; // (launch number << 32 | mover count), written by k_resort_scan_tiles into pinned, mapped host
    uint64_t *rsHostTotalDev = nullptr; // memory through this device pointer
    uint32_t rsSeq = 0;
    Event rsEvent;
    bool rsTilesDirty = false; // rsTileMovers holds counts no scan has consumed
    ResortStats rs; // steps, fallbacks, mover count of the last coherent re-sort (nrs_host_state.h)

    ResortScan scan_of_movers() const;
    ResortScan scan_of_dead() const;
    ResortOffsets offsets_movers() const { return ResortOffsets{rsTileOffset.as<uint32_t>(), rsGroupPrefix.as<uint32_t>()}; }
    int wait_mover_count(uint32_t *M);
};

} // namespace nrs
