// nrs_sort.hip — SortStage (nrs_sort.h): the radix sorts and the merge of the sort stage, the launches of the scan / split / dead-count
// kernels of the coherent re-sort (nrs_kernels_sort.h; scheme: nrs_kernels_resort.h), and the plain pair sort of the boundary code.
// The one translation unit of libnereus_hip.so that includes rocPRIM: its sorts are instantiated here once, not once per context type.
#include <sched.h>

#include "nrs_sort.h"
#include "nrs_kernels_sort.h"
#include <rocprim/rocprim.hpp>  // (behind nrs_ctx_base.h: it uses memset without including <cstring>)

namespace nrs {

// Radix sort of (hash, index) pairs.  rocPRIM's onesweep sorts 8 key bits per pass by default, so the 25-27-bit
// hashes of the dam-break grids take 4 passes; with 9 bits per pass they take 3.
using SortCfg9 = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                            rocprim::radix_sort_onesweep_config<rocprim::kernel_config<512, 12>, rocprim::kernel_config<512, 12>, 9,
                                                                                rocprim::block_radix_rank_algorithm::match>>;
using SortCfg10 = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                             rocprim::radix_sort_onesweep_config<rocprim::kernel_config<512, 12>, rocprim::kernel_config<512, 12>, 10,
                                                                                 rocprim::block_radix_rank_algorithm::match>>;
static inline hipError_t sort_pairs(void *tmp, size_t &bytes, rocprim::double_buffer<uint32_t> &k, rocprim::double_buffer<uint32_t> &v,
                                    size_t n, unsigned bits, hipStream_t stream)
{
    if (bits > 24 && bits <= 27) return rocprim::radix_sort_pairs<SortCfg9>(tmp, bytes, k, v, n, 0u, bits, stream);
    if (bits > 27 && bits <= 30) return rocprim::radix_sort_pairs<SortCfg10>(tmp, bytes, k, v, n, 0u, bits, stream);
    return rocprim::radix_sort_pairs(tmp, bytes, k, v, n, 0u, bits, stream);
}

// Radix sort of the movers of the coherent re-sort (nrs_kernels_resort.h): u64 keys "hash << 32 | slot", only the hash
// bits are sorted (the slots are already ascending and the sort is stable).  A few hundred thousand keys: onesweep
// from 8192 keys on (rocPRIM's default switches to its merge sort below 1 M keys: measured 104 vs 66 us at 300 k).
template <unsigned BITS>
using MoverSortCfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                                rocprim::radix_sort_onesweep_config<rocprim::kernel_config<512, 12>, rocprim::kernel_config<512, 12>, BITS,
                                                                                    rocprim::block_radix_rank_algorithm::match>, 8192>;
static inline hipError_t sort_movers(void *tmp, size_t &bytes, rocprim::double_buffer<uint64_t> &k, size_t m, unsigned bits, hipStream_t stream)
{
    if (bits > 24 && bits <= 27) return rocprim::radix_sort_keys<MoverSortCfg<9>>(tmp, bytes, k, m, 32u, 32u + bits, stream);
    if (bits > 27 && bits <= 30) return rocprim::radix_sort_keys<MoverSortCfg<10>>(tmp, bytes, k, m, 32u, 32u + bits, stream);
    return rocprim::radix_sort_keys<MoverSortCfg<8>>(tmp, bytes, k, m, 32u, 32u + bits, stream);
}

hipError_t sort_pairs_plain(void *tmp, size_t &bytes, PairBuffers &p, size_t n, unsigned bits, hipStream_t stream)
{
    rocprim::double_buffer<uint32_t> k(p.key, p.keyAlt), v(p.val, p.valAlt);
    const hipError_t e = rocprim::radix_sort_pairs(tmp, bytes, k, v, n, 0u, bits, stream);
    if (tmp && e == hipSuccess) p = PairBuffers{k.current(), k.alternate(), v.current(), v.alternate()};
    return e;
}

int SortStage::init(uint64_t cap, bool resort, hipStream_t s)
{
    stream = s;
    const size_t u = 4 * cap;
    NRSCHK(hashA.alloc(u)); NRSCHK(hashB.alloc(u)); NRSCHK(indexA.alloc(u)); NRSCHK(indexB.alloc(u));
    // radix sort workspace for the largest problem
    size_t tmp = 0;
    rocprim::double_buffer<uint32_t> k(hashA.as<uint32_t>(), hashB.as<uint32_t>());
    rocprim::double_buffer<uint32_t> vv(indexA.as<uint32_t>(), indexB.as<uint32_t>());
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp, k, vv, (size_t)cap, 0u, 32u, stream));
    size_t tmp9 = 0;
    HIPCHK(rocprim::radix_sort_pairs<SortCfg9>(nullptr, tmp9, k, vv, (size_t)cap, 0u, 27u, stream));
    size_t tmp10 = 0;
    HIPCHK(rocprim::radix_sort_pairs<SortCfg10>(nullptr, tmp10, k, vv, (size_t)cap, 0u, 30u, stream));
    size_t tmpAll = std::max(tmp, std::max(tmp9, tmp10));
    // coherent re-sort: steps on the production kernels re-use the previous step's order
    if (resort) {
        const size_t nTiles = (cap + BLOCK - 1) / BLOCK, nGroups = (nTiles + RESORT_GROUP - 1) / RESORT_GROUP;
        const size_t mcap = cap; // any share of the particles may be movers (RESORT_MAX_MOVER_PCT decides per step)
        NRSCHK(rsMovers.alloc(8 * cap)); NRSCHK(rsMoversAlt.alloc(8 * mcap)); NRSCHK(rsStayers.alloc(8 * cap)); NRSCHK(rsMerged.alloc(8 * cap));
        NRSCHK(rsTileMovers.alloc(4 * nTiles)); NRSCHK(rsTileOffset.alloc(4 * nTiles));
        NRSCHK(rsGroupTotal.alloc(4 * nGroups)); NRSCHK(rsGroupPrefix.alloc(4 * nGroups)); NRSCHK(rsScalars.alloc(16));
        NRSCHK(rsPrevPacked.alloc(4 * cap));
        NRSCHK(rsTileDead.alloc(4 * nTiles)); NRSCHK(rsTileDeadOffset.alloc(4 * nTiles));
        NRSCHK(rsGroupDeadTotal.alloc(4 * nGroups)); NRSCHK(rsGroupDeadPrefix.alloc(4 * nGroups));
        HIPCHK(hipMemsetAsync(rsTileDead.p, 0, 4 * nTiles, stream));
        HIPCHK(hipMemsetAsync(rsTileMovers.p, 0, 4 * nTiles, stream));
        HIPCHK(hipMemsetAsync(rsScalars.p, 0, 16, stream));
        HIPCHK(hipHostMalloc((void **)&rsHostTotal.p, 64, hipHostMallocMapped));
        std::memset(rsHostTotal, 0, 64);
        HIPCHK(hipHostGetDevicePointer((void **)&rsHostTotalDev, rsHostTotal, 0));
        HIPCHK(hipEventCreateWithFlags(&rsEvent.e, hipEventDisableTiming));
        rocprim::double_buffer<uint64_t> mk(rsMovers.as<uint64_t>(), rsMoversAlt.as<uint64_t>());
        for (unsigned bits : {24u, 27u, 30u}) {
            size_t t = 0;
            HIPCHK(sort_movers(nullptr, t, mk, mcap, bits, stream));
            tmpAll = std::max(tmpAll, t);
        }
        size_t t = 0;
        HIPCHK(rocprim::merge(nullptr, t, rsStayers.as<uint64_t>(), rsMovers.as<uint64_t>(), rsMerged.as<uint64_t>(), (size_t)cap, mcap,
                              rocprim::less<uint64_t>(), stream));
        tmpAll = std::max(tmpAll, t);
    }
    NRSCHK(sortTmp.alloc(tmpAll));
    return NRS_OK;
}

int SortStage::sort_keys(const SortPrefix &c, uint32_t N, unsigned bits, const uint64_t **mergedOut)
{
    const uint64_t *merged = nullptr;
    if (c.resort) {
        // the split of these keys into movers / stayers was queued behind the kernel that wrote them; its mover count sizes
        // the mover sort and the merge (see nrs_kernels_resort.h)
        uint32_t M = c.knownCount; // (slab runs: the host already has the mover count)
        if (!c.countKnown) NRSCHK(wait_mover_count(&M));
        SortKind kind;
        NRSCHK(choose_sort(M, N, rs, kind));
        if (kind == SortKind::MERGE_STAYERS) {
            merged = rsStayers.as<uint64_t>();
        } else if (kind == SortKind::MERGE_MOVERS) {
            rocprim::double_buffer<uint64_t> mk(rsMovers.as<uint64_t>(), rsMoversAlt.as<uint64_t>());
            size_t tmp = sortTmp.bytes;
            HIPCHK(sort_movers(sortTmp.p, tmp, mk, (size_t)M, bits, stream));
            tmp = sortTmp.bytes;
            HIPCHK(rocprim::merge(sortTmp.p, tmp, rsStayers.as<uint64_t>(), mk.current(), rsMerged.as<uint64_t>(), (size_t)(N - M),
                                  (size_t)M, rocprim::less<uint64_t>(), stream));
            merged = rsMerged.as<uint64_t>();
        }
    }
    const KeyPair alt = next_keys();
    if (!merged) {
        if (!c.resort) rs.lastMovers = -1.0;
        rocprim::double_buffer<uint32_t> k(hashCur, alt.hash);
        rocprim::double_buffer<uint32_t> v(indexCur, alt.index);
        size_t tmp = sortTmp.bytes;
        HIPCHK(sort_pairs(sortTmp.p, tmp, k, v, (size_t)N, bits, stream));
        hashCur = k.current(); indexCur = v.current();
    } else {
        hashCur = alt.hash; indexCur = alt.index; // plain sorted arrays, written by k_reorder_merged
    }
    *mergedOut = merged;
    return NRS_OK;
}

int SortStage::clean_tile_counts()
{
    if (rsTilesDirty) {
        HIPCHK(hipMemsetAsync(rsTileMovers.p, 0, rsTileMovers.bytes, stream));
        HIPCHK(hipMemsetAsync(rsTileDead.p, 0, rsTileDead.bytes, stream));
    }
    rsTilesDirty = false;
    return NRS_OK;
}

ResortScan SortStage::scan_of_movers() const
{
    uint32_t *sc = rsScalars.as<uint32_t>();
    return ResortScan{rsTileMovers.as<uint32_t>(), rsTileOffset.as<uint32_t>(), rsGroupTotal.as<uint32_t>(), rsGroupPrefix.as<uint32_t>(), sc + 1};
}
ResortScan SortStage::scan_of_dead() const
{
    uint32_t *sc = rsScalars.as<uint32_t>();
    return ResortScan{rsTileDead.as<uint32_t>(), rsTileDeadOffset.as<uint32_t>(), rsGroupDeadTotal.as<uint32_t>(), rsGroupDeadPrefix.as<uint32_t>(), sc + 2};
}

int SortStage::scan_tiles(const ResortScan &a, uint32_t *done, uint32_t nTiles) const
{
    const uint32_t nGroups = (nTiles + RESORT_GROUP - 1) / RESORT_GROUP;
    hipLaunchKernelGGL(k_resort_scan_tiles, dim3(nGroups), dim3(RESORT_GROUP), 0, stream, a, ResortScan{}, done, (volatile uint64_t *)nullptr, 0u, nTiles);
    return NRS_OK;
}

int SortStage::scan_movers(uint32_t nTiles, bool withDead)
{
    const uint32_t nGroups = (nTiles + RESORT_GROUP - 1) / RESORT_GROUP;
    hipLaunchKernelGGL(k_resort_scan_tiles, dim3(nGroups), dim3(RESORT_GROUP), 0, stream, scan_of_movers(), withDead ? scan_of_dead() : ResortScan{},
                       rsScalars.as<uint32_t>(), (volatile uint64_t *)rsHostTotalDev, ++rsSeq, nTiles);
    HIPCHK(hipEventRecord(rsEvent, stream));
    rsTilesDirty = false; // the scan resets the counts it reads
    return NRS_OK;
}

int SortStage::scan_holes(uint32_t N)
{
    NRSCHK(clean_tile_counts());
    hipLaunchKernelGGL(k_holes_count, dim3(nblocks(N)), dim3(BLOCK), 0, stream, hashNext, rsTileDead.as<uint32_t>(), N);
    return scan_tiles(scan_of_dead(), rsScalars.as<uint32_t>(), nblocks(N));
}

int SortStage::split(SplitFrom from, uint32_t N, uint32_t *clearCells)
{
    const uint32_t *prev = from == SplitFrom::PACKED ? rsPrevPacked.as<uint32_t>() : hashCur;
    const dim3 g(nblocks(N)), b(BLOCK);
    if (from == SplitFrom::SORTED_HOLES)
        hipLaunchKernelGGL((k_resort_split<true>), g, b, 0, stream, prev, hashNext, offsets_movers(), offsets_dead(), rsMovers.as<uint64_t>(),
                           rsStayers.as<uint64_t>(), N, clearCells);
    else
        hipLaunchKernelGGL((k_resort_split<false>), g, b, 0, stream, prev, hashNext, offsets_movers(), offsets_movers(), rsMovers.as<uint64_t>(),
                           rsStayers.as<uint64_t>(), N, clearCells);
    return NRS_OK;
}

// The scan kernel stores (launch number, count) straight into mapped host memory; polling that word costs a PCIe
// write latency, where hipEventSynchronize on an otherwise idle host thread was measured to cost ~0.1 ms per step.
int SortStage::wait_mover_count(uint32_t *M)
{
    volatile uint64_t *w = (volatile uint64_t *)rsHostTotal;
    for (uint64_t spins = 0;; ++spins) {
        const uint64_t v = *w;
        if ((uint32_t)(v >> 32) == rsSeq) { *M = (uint32_t)v; return NRS_OK; }
        // polite spin: on a host with fewer free cores than ranks (8 ranks on a 16-CPU share) the poller hands its
        // time slice to whoever is runnable; with an idle core the yield returns at once and costs no latency
        if ((spins & 63u) == 63u) sched_yield();
        if ((spins & 0xfffff) == 0xfffff) { // every ~1 M polls: has the stream failed or finished without us seeing it?
            const hipError_t e = hipEventQuery(rsEvent);
            if (e == hipSuccess) break;
            if (e != hipErrorNotReady) HIPCHK(e);
        }
    }
    HIPCHK(hipEventSynchronize(rsEvent));
    *M = (uint32_t)*w;
    return NRS_OK;
}

} // namespace nrs
