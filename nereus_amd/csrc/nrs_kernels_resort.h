// nrs_kernels_resort.h — coherent re-sort of the (hash, index) pairs between two steps.
//
// The reference sorts all pairs from scratch every step (thrust::sort_by_key, sph_cuda.cu:310-313).  Between two
// steps only a few per cent of the particles change grid cell (CFL: < 1 cell per step; measured 0.3-7 % over the
// first 400 steps of the 1 M dam-break), and the arrays are still in the previous step's sorted order.  With
// k_i = next hash of the particle in sorted slot i, the stable sort by (k_i, i) is therefore a MERGE of
//   stayers  (k_i == previous hash of slot i): already sorted, because their keys are the previous sorted keys,
//   movers   (k_i != previous hash):           few; sorted on their own with a radix sort.
// Pairs travel as one u64 "hash << 32 | slot" so that the merge order IS the stable-sort order (no ties); the
// result is identical to the full stable radix sort, element for element.
//
//   k_forces_*  (fused epilogue)   counts the movers of every 256-slot tile            → tileMovers[tile]
//   k_resort_scan_tiles            exclusive scan of the tile counts, total to the host → tileOffset[], *total
//   k_resort_split                 stable two-way compaction into movers[] / stayers[]
//   radix sort of the keys         movers only (bits 32 .. 32+log2(numCells))
//   merge                          stayers + movers → merged[]
//   k_reorder_merged               cell ranges + gather from merged[], also leaves plain hash[] / index[] arrays
// Everything up to the merge needs no precision: SortStage (nrs_sort.h) owns the buffers and nrs_sort.hip holds those kernels and
// calls.  Here: the two kernels that move particle data, k_holes_compact and k_reorder_merged.
// The host needs the mover count to size the last two calls: it is read after the split has been queued, so the
// copy overlaps the split and the cell-table reset; above RESORT_MAX_MOVER_PCT % movers the step falls back to the full
// radix sort.
#pragma once
#include "nrs_kernels_ref.h"
#include "nrs_sort.h"

namespace nrs {

// stable compaction of (pos, vel) by "slot is live", used when somebody looks at the arrays while they have holes
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_holes_compact(const uint32_t *__restrict__ keys, ResortOffsets dead,
                                                         const typename Vec4T<R>::type *__restrict__ pos,
                                                         const typename Vec4T<R>::type *__restrict__ vel,
                                                         typename Vec4T<R>::type *__restrict__ outPos,
                                                         typename Vec4T<R>::type *__restrict__ outVel, uint32_t n)
{
    __shared__ uint32_t waveCount[BLOCK / 64];
    const uint32_t tile = blockIdx.x, tid = threadIdx.x;
    const uint32_t i = tile * BLOCK + tid;
    const bool hole = i < n && keys[i] == 0xffffffffu;
    const uint64_t hmask = __ballot(hole);
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    if (lane == 0) waveCount[wave] = (uint32_t)__popcll(hmask);
    __syncthreads();
    uint32_t hbefore = (uint32_t)__popcll(hmask & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) hbefore += waveCount[w];
    if (i >= n || hole) return;
    const uint32_t d = i - (dead.groupPrefix[tile / RESORT_GROUP] + dead.tileOffset[tile] + hbefore);
    outPos[d] = pos[i];
    outVel[d] = vel[i];
}

// reorderDataAndFindCellStartD (sph_kernel_impl.cuh:210-281) fed by the merged u64 pairs; also writes the plain
// sorted hash / index arrays the rest of the step (and nrs_get_array) use.
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_reorder_merged(const uint64_t *__restrict__ merged, uint32_t *__restrict__ hashOut,
                                                          uint32_t *__restrict__ indexOut,
                                                          const typename Vec4T<R>::type *__restrict__ oldPos,
                                                          const typename Vec4T<R>::type *__restrict__ oldVel,
                                                          const R *__restrict__ oldPres,
                                                          typename Vec4T<R>::type *__restrict__ sPos,
                                                          typename Vec4T<R>::type *__restrict__ sVel, R *__restrict__ sPres,
                                                          uint32_t *__restrict__ cellStart, uint32_t *__restrict__ cellEnd,
                                                          uint32_t *__restrict__ inv, uint32_t n,
                                                          const uint32_t *__restrict__ nearBits, uint32_t *__restrict__ wallTileCount,
                                                          unsigned long long *__restrict__ wallMask, QuantCfg qc, qword_t *__restrict__ qpos)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const uint64_t e = i < n ? merged[i] : 0ull;
    const uint32_t h = (uint32_t)(e >> 32), src = (uint32_t)e;
    typename Vec4T<R>::type p4 = mk4<R>((R)0, (R)0, (R)0, (R)0);
    if (i < n) p4 = oldPos[src];
    if (nearBits) wall_tile_count(nearBits, wallTileCount, h, i < n, wallMask, qpos && quant_far<R>(qc, xyz<R>(p4))); // (far owners: see k_reorder)
    if (i >= n) return;
    if (i == 0) {
        cellStart[h] = 0;
    } else {
        const uint32_t hp = (uint32_t)(merged[i - 1] >> 32);
        if (h != hp) { cellStart[h] = i; cellEnd[hp] = i; }
    }
    if (i == n - 1) cellEnd[h] = n;
    hashOut[i] = h;
    indexOut[i] = src;
    sPos[i] = p4;
    if (qpos) qpos[i] = quantize_pos<R>(qc, xyz<R>(p4));
    sVel[i] = oldVel[src];
    if (oldPres) sPres[i] = oldPres[src];
    if (inv) inv[src] = i;
}

} // namespace nrs
