// nrs_kernels_sort.h — the three kernels of the coherent re-sort (scheme: nrs_kernels_resort.h) that need no precision: the scan of the
// per-tile counts, the split into movers / stayers, the count of dead slots.  SortStage (nrs_sort.h) owns their buffers; nrs_sort.hip
// is the one unit of the library that includes this header and launches them (tools/bench_coherent_sort.hip times them on its own).
#pragma once
#include "nrs_math.h"
#include "nrs_sort.h"

namespace nrs {

// Exclusive scan of the per-tile mover counts, two levels: every workgroup scans RESORT_GROUP counts (coalesced; the
// counts are reset to 0 for the next step's atomics) and the last one to finish scans the group totals.
// tileOffset[t] is local to the group; groupPrefix[t / RESORT_GROUP] is added by the consumer.
static __global__ __launch_bounds__(RESORT_GROUP) void k_resort_scan_tiles(ResortScan a, ResortScan b, uint32_t *__restrict__ done,
                                                                     volatile uint64_t *hostTotal, uint32_t seq, uint32_t nTiles)
{
    // a = movers (always), b = dead slots (slab runs that leave holes; b.tile == nullptr otherwise).  The total of `a`
    // goes to the host.
    __shared__ uint32_t waveSum[RESORT_GROUP / 64];
    __shared__ bool last;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    auto block_exclusive = [&](uint32_t v, uint32_t &sum) { // exclusive prefix of v over the workgroup, sum = total
        uint32_t inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d);
            if (lane >= (uint32_t)d) inc += o;
        }
        __syncthreads();
        if (lane == 63) waveSum[wave] = inc;
        __syncthreads();
        uint32_t base = 0, all = 0;
        for (uint32_t w = 0; w < RESORT_GROUP / 64; ++w) { const uint32_t c = waveSum[w]; if (w < wave) base += c; all += c; }
        sum = all;
        return base + inc - v;
    };
    const uint32_t t = blockIdx.x * RESORT_GROUP + tid;
    const ResortScan arr[2] = {a, b};
    for (int k = 0; k < 2; ++k) {
        if (!arr[k].tile) continue;
        uint32_t v = 0;
        if (t < nTiles) { v = arr[k].tile[t]; arr[k].tile[t] = 0; }
        uint32_t sum;
        const uint32_t ex = block_exclusive(v, sum);
        if (t < nTiles) arr[k].tileOffset[t] = ex;
        if (tid == 0) arr[k].groupTotal[blockIdx.x] = sum;
    }
    if (tid == 0) {
        __threadfence();
        last = atomicAdd(done, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    // gridDim.x <= RESORT_GROUP (checked by the host): one more scan over the group totals
    for (int k = 0; k < 2; ++k) {
        if (!arr[k].tile) continue;
        const uint32_t g = tid < gridDim.x ? __atomic_load_n(&arr[k].groupTotal[tid], __ATOMIC_RELAXED) : 0u;
        uint32_t all;
        const uint32_t gex = block_exclusive(g, all);
        if (tid < gridDim.x) arr[k].groupPrefix[tid] = gex;
        if (tid == 0) {
            *arr[k].total = all;
            if (k == 0 && hostTotal) *hostTotal = ((uint64_t)seq << 32) | all; // one 8-byte store to mapped host memory: (launch number, count)
        }
    }
    if (tid == 0) *done = 0;
}

// stable split of slot i (tile = i / BLOCK) by "hash changed": movers[rank among movers], stayers[rank among stayers].
// HOLES (slab runs that do not compact their arrays): a slot whose next key is 0xffffffff is dead (its particle left
// the slab or was a halo copy) and goes to neither list; `dead` holds the scanned per-tile counts of such slots.
template <bool HOLES>
__global__ __launch_bounds__(BLOCK) void k_resort_split(const uint32_t *__restrict__ prevHash, const uint32_t *__restrict__ nextHash,
                                                        ResortOffsets mov, ResortOffsets dead, uint64_t *__restrict__ movers,
                                                        uint64_t *__restrict__ stayers, uint32_t n, uint32_t *__restrict__ clearCells)
{
    // clearCells (cellStart, or null): also undo the cell table of the step that just ended — the work of k_clear_cells
    // (nrs_kernels_ref.h), folded in here because this kernel reads the step's sorted keys anyway and runs after every
    // reader of the table
    __shared__ uint32_t waveCount[2][BLOCK / 64];
    const uint32_t tile = blockIdx.x, tid = threadIdx.x;
    const uint32_t i = tile * BLOCK + tid;
    const bool live = i < n;
    uint32_t k = 0;
    bool mover = false, hole = false;
    if (live) {
        k = nextHash[i];
        hole = HOLES && k == 0xffffffffu;
        const uint32_t prev = prevHash[i];
        mover = !hole && k != prev;
        if (clearCells && (i == 0 || prev != prevHash[i - 1])) clearCells[prev] = CELL_EMPTY;
    }
    const uint64_t mask = __ballot(mover), hmask = HOLES ? __ballot(hole) : 0ull;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    if (lane == 0) { waveCount[0][wave] = (uint32_t)__popcll(mask); waveCount[1][wave] = (uint32_t)__popcll(hmask); }
    __syncthreads();
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t before = (uint32_t)__popcll(mask & below), hbefore = (uint32_t)__popcll(hmask & below);
    for (uint32_t w = 0; w < wave; ++w) { before += waveCount[0][w]; hbefore += waveCount[1][w]; }
    if (!live || hole) return;
    const uint32_t moversBefore = mov.groupPrefix[tile / RESORT_GROUP] + mov.tileOffset[tile] + before;
    const uint32_t holesBefore = HOLES ? dead.groupPrefix[tile / RESORT_GROUP] + dead.tileOffset[tile] + hbefore : 0u;
    const uint64_t e = ((uint64_t)k << 32) | i;
    if (mover) movers[moversBefore] = e;
    else stayers[i - moversBefore - holesBefore] = e;
}

// per-tile count of dead slots (input of the scan that k_holes_compact needs)
static __global__ __launch_bounds__(BLOCK) void k_holes_count(const uint32_t *__restrict__ keys, uint32_t *__restrict__ tileDead, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const uint64_t m = __ballot(i < n && keys[i] == 0xffffffffu);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(&tileDead[blockIdx.x], (uint32_t)__popcll(m));
}

} // namespace nrs
