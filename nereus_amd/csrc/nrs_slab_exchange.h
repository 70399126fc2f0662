// nrs_slab_exchange.h — the device half of the slab exchange (nrs_slab_configure / _pack / _unpack): the cuts, the host decisions
// with what the last pack left (SlabHost, nrs_host_slab.h), the ghost streams, the block counts, stream totals and classification
// flags of the partition, the page-locked landing of everything the host reads in an exchange and the event behind the pack's part of
// it.  It launches the kernels of nrs_kernels_slab.h, which take Params<R> and vec4 pointers only: it depends on the precision alone.
// The context (nrs_ctx_impl.h) holds one, reads it through the views below and calls its operations with the particle arrays and
// the sort stage of the moment; it keeps n, nOwned, the state of the particle arrays (st) and everything a refusal is decided from.
#pragma once
#include <climits>

#include "nrs_ctx_base.h"
#include "nrs_host_slab.h"
#include "nrs_kernels_slab.h"
#include "nrs_sort.h"

namespace nrs {

static_assert(SLT_STAY == ST_STAY && SLT_MIG_L == ST_MIG_L && SLT_HALO_L == ST_HALO_L && SLT_MIG_R == ST_MIG_R && SLT_HALO_R == ST_HALO_R &&
              SLT_GHOST == ST_GHOST && SLT_COUNT == ST_COUNT && SLT_CHANGED == ST_CHANGED && SLT_TOTALS == ST_TOTALS,
              "nrs_host_slab.h numbers the stream totals as nrs_kernels_slab.h does");

// fused classification: where the force kernel of a step writes its stream flags and stream populations (FusedOut)
struct SlabClassify {
    uint8_t *flags;        // per slot
    uint32_t *blockCounts; // ST_TOTALS rows of `blocks` counts, zeroed
    uint32_t blocks;       // SLAB_TILE slots each
};

template <typename R> struct SlabExchange {
    typedef typename Vec4T<R>::type T4;

    // the capacity of the particle arrays; every later launch, memset, copy and event record goes to `stream`
    void init(uint64_t cap_, hipStream_t stream_) { cap = cap_; stream = stream_; }

    // ---- views -----------------------------------------------------------------------------------------------------------------------
    bool on() const { return slabOn; }                 // nrs_slab_configure has been called
    const SlabCfg &cuts() const { return slab; }       // [lo, hi) in global cell-x, and the halo width
    const SlabHost &host() const { return sx; }        // the window, the last pack and its totals
    int max_iters() const { return (slab.halo - 4) / 2; } // IISPH solver iterations the halo supports

    // ---- nrs_slab_configure, after its refusals: the cuts; *cutsChanged: they differ from the ones before -------------------------
    void configure(int lo, int hi, int halo, bool *cutsChanged)
    {
        *cutsChanged = slab.lo != lo || slab.hi != hi || slab.halo != halo;
        slab.lo = lo; slab.hi = hi; slab.halo = halo;
        slabOn = true;
    }
    // cell-table window of this rank for the cuts; true when it changed (SlabHost::choose_window)
    bool choose_window(const uint32_t grid[3], bool force) { return sx.choose_window(grid, slab.lo, slab.hi, slab.halo, force); }

    // ---- fused classification: the flags and zeroed block counts the force kernel of a step of N particles writes ------------------
    int classify_targets(uint32_t N, SlabClassify &out)
    {
        const uint32_t nbk = pack_blocks(N);
        NRSCHK(slabFlags.alloc(cap));
        NRSCHK(ensure_counts(nbk));
        HIPCHK(hipMemsetAsync(slabCounts.p, 0, (size_t)ST_TOTALS * nbk * 4, stream));
        out.flags = slabFlags.as<uint8_t>();
        out.blockCounts = slabCounts.as<uint32_t>();
        out.blocks = nbk;
        return NRS_OK;
    }

    // ---- nrs_slab_pack, from the chosen form to the queued totals: count -> scan -> scatter, the headers, the totals on their way to
    // the host and, in place, the split of the slots that stay.  posA / velA: the N current particles; posB / velB: where a compacting
    // partition puts the ones that stay.  Nothing waits.
    int pack(const Params<R> &P, T4 *posA, T4 *velA, T4 *posB, T4 *velB, uint32_t N, void *sendL, void *sendR, uint64_t mcap, SlabChoice ch,
             SortStage &sort)
    {
        const uint32_t nbk = pack_blocks(N);
        NRSCHK(ensure_counts(nbk));
        NRSCHK(slabTotals.alloc(ST_TOTALS * 4));
        NRSCHK(ghostPos.alloc(sizeof(T4) * mcap));
        NRSCHK(ghostVel.alloc(sizeof(T4) * mcap));
        NRSCHK(ensure_host_totals());
        NRSCHK(ensure_pack_event());
        const bool inplace = ch.form != SlabForm::COMPACT, pre = ch.form == SlabForm::PRECLASSIFIED;
        if (N) {
            // pre-classified: the force kernel of the last step classified every slot for these cuts (flags, stream populations per
            // 2048 slots, dead marks in the keys, movers / dead per 256 slots); what is left is to scan, copy out the few particles
            // of the message and ghost streams, and split
            if (!pre)
                hipLaunchKernelGGL((k_slab_count<R>), dim3(nbk), dim3(SLAB_BLOCK), 0, stream, P, slab, posA, N,
                                   slabCounts.as<uint32_t>(), nbk, ch.resort ? sort.hash() : (const uint32_t *)nullptr,
                                   ch.resort ? sort.prepared().hash : (const uint32_t *)nullptr);
            hipLaunchKernelGGL(k_slab_scan, dim3(ST_TOTALS), dim3(SLAB_BLOCK), 0, stream, slabCounts.as<uint32_t>(), nbk, slabTotals.as<uint32_t>());
            // in place, the fused kernel's keys / slot numbers stay where they are; the compacting form does the hash pass of the next
            // step here, into the key buffers the last sort did not end in
            const KeyPair target = sort.pack_targets(inplace);
            SlabOut<R> out;
            out.stayPos = posB; out.stayVel = velB;
            out.hash = target.hash; out.index = target.index;
            out.prevHash = ch.resort ? sort.hash() : nullptr;
            out.prevPacked = (ch.resort && !inplace) ? sort.prev_packed() : nullptr;
            out.tileMovers = ch.resort ? sort.tile_movers() : nullptr;
            out.tileDead = inplace ? sort.tile_dead() : nullptr;
            out.flags = pre ? slabFlags.as<uint8_t>() : nullptr;
            out.ghostPos = ghostPos.as<T4>(); out.ghostVel = ghostVel.as<T4>();
            out.sendL = (unsigned char *)sendL; out.sendR = (unsigned char *)sendR;
            out.cap = (uint32_t)mcap;
            if (ch.resort && !pre) { // the scatter counts per tile (pre-classified: the force kernel did, and its counts are still there)
                NRSCHK(sort.clean_tile_counts());
                sort.tile_counts_written(); // (and stay marked until a scan: the counts of an unused classification may still be in the arrays)
            }
            const auto scatter = pre ? k_slab_scatter<R, true, true> : inplace ? k_slab_scatter<R, true> : k_slab_scatter<R, false>;
            hipLaunchKernelGGL(scatter, dim3(nbk), dim3(SLAB_BLOCK), 0, stream, P, slab, posA, velA, N, slabCounts.as<uint32_t>(),
                               nbk, slabTotals.as<uint32_t>(), out);
        } else {
            HIPCHK(hipMemsetAsync(slabTotals.p, 0, ST_TOTALS * 4, stream));
        }
        hipLaunchKernelGGL(k_slab_headers, dim3(1), dim3(64), 0, stream, slabTotals.as<uint32_t>(), (unsigned char *)sendL, (unsigned char *)sendR);
        HIPCHK(hipGetLastError());
        // In place, the split of the slots we keep does not depend on what arrives: it is queued now, so that it runs while the
        // messages travel.  Its scan also totals the cell changers and the dead slots, which in the pre-classified form nothing else
        // has counted: there the scan comes before the copy and the event.  Otherwise the event comes first, and finish() never
        // waits for the scan.  (N == 0: the totals are zero and nobody reads the landing; only the event is needed.)
        const uint32_t nTiles = nblocks(N);
        if (!N) HIPCHK(hipEventRecord(packEvent, stream));
        else if (!pre) NRSCHK(totals_to_host(false, sort));
        if (inplace) NRSCHK(sort.scan_movers(nTiles, true));
        if (pre) NRSCHK(totals_to_host(true, sort));
        if (inplace) {
            NRSCHK(sort.split(SplitFrom::SORTED_HOLES, N, nullptr));
            HIPCHK(hipGetLastError());
        }
        // Nothing above waits.  The messages are complete in stream order, so the caller can enqueue its sends right behind this call;
        // the stream totals (how many stay, leave, ghost) are read back by finish() — in nrs_slab_unpack, together with the
        // headers of the received messages: ONE host synchronisation per exchange instead of two — or by whichever entry point needs
        // the particle count first (settle()).
        sx.queue(ch, N, mcap);
        return NRS_OK;
    }
    // ---- the host half of the pack, run when the stream totals are needed: nothing if no pack is pending, else the wait for its event
    // and SlabHost::finish on the landed words (f.stored: the context applies them)
    int finish(SlabFinish &f)
    {
        f = SlabFinish();
        if (!sx.pending) return NRS_OK;
        sx.pending = false; // (whatever the wait returns)
        HIPCHK(hipEventSynchronize(packEvent));
        return sx.finish(slabHostTotals + HT_TOTALS, slabHostTotals[HT_SCAN_CHANGED], slabHostTotals[HT_SCAN_DEAD], f);
    }

    // ---- nrs_slab_unpack -----------------------------------------------------------------------------------------------------------
    // ONE host synchronisation for the exchange: the headers of the received messages (how many migrants, how many halo copies)
    // are copied to page-locked memory behind the receives, and the same wait covers the stream totals of the pack (finish).
    // *hL / *hR: the four words of each header, null for a missing message.
    int read_headers(const void *recvL, const void *recvR, const uint32_t **hL, const uint32_t **hR)
    {
        NRSCHK(ensure_host_totals());
        *hL = recvL ? slabHostTotals + HT_HEADER_L : nullptr; *hR = recvR ? slabHostTotals + HT_HEADER_R : nullptr;
        if (*hL) HIPCHK(hipMemcpyAsync(slabHostTotals + HT_HEADER_L, recvL, 16, hipMemcpyDeviceToHost, stream));
        if (*hR) HIPCHK(hipMemcpyAsync(slabHostTotals + HT_HEADER_R, recvR, 16, hipMemcpyDeviceToHost, stream));
        if (*hL || *hR) HIPCHK(hipStreamSynchronize(stream));
        return NRS_OK;
    }
    // where the pieces go (SlabHost::unpack); n, physN, holes: the context's live count, the extent of its arrays, whether they have holes
    int arrivals(const uint32_t *hL, const uint32_t *hR, uint64_t n, uint32_t physN, bool holes, uint64_t mcap, SlabArrivals &ar) const
    {
        return sx.unpack(hL, hR, n, physN, holes, mcap, cap, ar);
    }
    // the migrants, our ghosts and the halo copies behind the particles that stayed.  compactResort: a compacting form with a re-sort,
    // the append extends the compacted old keys and the tile counts of the scatter; knownMovers: in place, the movers counted so far
    int append(const Params<R> &P, const SlabArrivals &ar, const void *recvL, const void *recvR, uint64_t mcap, T4 *posA, T4 *velA, SortStage &sort,
               bool compactResort, uint32_t knownMovers)
    {
        const unsigned char *bL = (const unsigned char *)recvL, *bR = (const unsigned char *)recvR;
        const uint32_t migL = bL ? slabHostTotals[HT_HEADER_L] : 0u, migR = bR ? slabHostTotals[HT_HEADER_R] : 0u;
        AppendPieces<R> A;
        A.srcPos[0] = bL ? msg(bL, 0, mcap) : nullptr;          A.srcVel[0] = bL ? msg(bL, 1, mcap) : nullptr;          // migrants from the left
        A.srcPos[1] = bR ? msg(bR, 0, mcap) : nullptr;          A.srcVel[1] = bR ? msg(bR, 1, mcap) : nullptr;          // migrants from the right
        A.srcPos[2] = ghostPos.as<T4>();                        A.srcVel[2] = ghostVel.as<T4>();                        // our ghosts
        A.srcPos[3] = bL ? msg(bL, 0, mcap) + migL : nullptr;   A.srcVel[3] = bL ? msg(bL, 1, mcap) + migL : nullptr;   // halo from the left
        A.srcPos[4] = bR ? msg(bR, 0, mcap) + migR : nullptr;   A.srcVel[4] = bR ? msg(bR, 1, mcap) + migR : nullptr;   // halo from the right
        std::memcpy(A.start, ar.start, sizeof(A.start));
        if (A.start[5])
            hipLaunchKernelGGL((k_slab_append<R>), dim3((A.start[5] + SLAB_BLOCK - 1) / SLAB_BLOCK), dim3(SLAB_BLOCK), 0, stream, P, A,
                               posA, velA, sort.pack_keys().hash, sort.pack_keys().index,
                               compactResort ? sort.prev_packed() : (uint32_t *)nullptr,
                               compactResort ? sort.tile_movers() : (uint32_t *)nullptr, (uint32_t)ar.base,
                               ar.inplace ? sort.movers() : (uint64_t *)nullptr, knownMovers);
        HIPCHK(hipGetLastError());
        return NRS_OK;
    }
    void unpack_done() { sx.resort = false; } // the unpack has used the last pack's SlabChoice::resort

    // ---- nrs_slab_histogram: particles per cell-x column from lo0 on, to the host; it waits -------------------------------------------
    int histogram(const Params<R> &P, const T4 *pos, uint64_t n, int lo0, uint32_t nbins, uint32_t *out)
    {
        DevBuf bins;
        NRSCHK(bins.alloc((size_t)nbins * 4));
        HIPCHK(hipMemsetAsync(bins.p, 0, (size_t)nbins * 4, stream));
        if (n)
            hipLaunchKernelGGL((k_slab_histogram<R>), dim3((uint32_t)((n + SLAB_BLOCK - 1) / SLAB_BLOCK)), dim3(SLAB_BLOCK), 0, stream, P,
                               pos, (uint32_t)n, lo0, nbins, bins.as<uint32_t>());
        HIPCHK(hipMemcpyAsync(out, bins.p, (size_t)nbins * 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return NRS_OK;
    }

private:
    hipStream_t stream = nullptr;
    uint64_t cap = 0;
    bool slabOn = false;
    SlabCfg slab = {INT_MIN / 2, INT_MAX / 2, 2};
    SlabHost sx;
    DevBuf ghostPos, ghostVel, slabCounts, slabTotals;
    DevBuf slabFlags; // fused classification: the force kernel's stream flags (the context's st: classifiedValid, classifiedN)
    // page-locked landing place (HT_WORDS words) of what the host reads in an exchange, and the event behind the pack's part of it
    enum { HT_TOTALS = 0,              // the ST_TOTALS stream totals of the pack
           HT_SCAN = 8,                // pre-classified form: sort.scan_scalars(), of which ...
           HT_SCAN_CHANGED = HT_SCAN + 1, HT_SCAN_DEAD = HT_SCAN + 2, // ... the cell changers and the dead slots
           HT_HEADER_L = 16, HT_HEADER_R = 20, // the 16-byte headers of the received messages
           HT_WORDS = 32 };
    PinnedBuf<uint32_t> slabHostTotals;
    Event packEvent;

    static uint32_t pack_blocks(uint32_t N) { return std::max<uint32_t>(1u, (N + SLAB_TILE - 1) / SLAB_TILE); }
    uint32_t cap_blocks() const { return (uint32_t)((cap + SLAB_TILE - 1) / SLAB_TILE); }
    // the block counts of a partition of nbk blocks: sized for the capacity at once, so that a growing N does not reallocate
    int ensure_counts(uint32_t nbk) { return slabCounts.alloc((size_t)ST_TOTALS * ((cap_blocks() > nbk) ? cap_blocks() : nbk) * 4); }
    int ensure_host_totals()
    {
        if (!slabHostTotals) HIPCHK(hipHostMalloc((void **)&slabHostTotals.p, HT_WORDS * 4, hipHostMallocDefault));
        return NRS_OK;
    }
    int ensure_pack_event()
    {
        if (!packEvent) HIPCHK(hipEventCreateWithFlags(&packEvent.e, hipEventDisableTiming));
        return NRS_OK;
    }
    // The stream totals (and, in the pre-classified form, the scalars of the re-sort's scan) on their way to the host, and the event
    // finish() waits for.  Page-locked destination: the copy is complete when the event behind it is (a pageable destination is
    // only guaranteed after a stream synchronization, which would also wait for the split queued behind it).
    int totals_to_host(bool withScan, const SortStage &sort)
    {
        HIPCHK(hipMemcpyAsync(slabHostTotals + HT_TOTALS, slabTotals.p, ST_TOTALS * 4, hipMemcpyDeviceToHost, stream));
        if (withScan) HIPCHK(hipMemcpyAsync(slabHostTotals + HT_SCAN, sort.scan_scalars(), 16, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipEventRecord(packEvent, stream));
        return NRS_OK;
    }
    // the positions (which = 0) or velocities (1) of a received message: behind its 16-byte header, mcap particles each
    static const T4 *msg(const unsigned char *b, int which, uint64_t mcap) { return (const T4 *)(b + 16 + (size_t)which * (size_t)mcap * sizeof(T4)); }
};

} // namespace nrs
