// nrs_wall_list.h — the step's wall list (wall-particle deferral, nrs_kernels_tiled.h): the sorted slots whose cell has the
// near-boundary bit that the boundary tables keep, found anew every step: the reorder kernel counts them per tile and marks them per
// slot, a two-level scan (the re-sort's scan kernel) turns the counts into offsets, k_wall_compact writes the list.  The buffers are
// sized by the fluid's capacity and depend on neither the precision nor the kernel set: the context (nrs_ctx_impl.h) holds one
// WallLists, hands its tile counts and slot masks to the reorder kernels and its view to the kernels with wall workgroups.
#pragma once
#include "nrs_ctx_base.h"
#include "nrs_kernels_ref.h"
#include "nrs_kernels_tiled.h"
#include "nrs_sort.h"

namespace nrs {

struct WallLists {
    // sized by the fluid capacity; a rest build of the boundary tables calls it where the near bits become valid
    int ensure(uint64_t cap, hipStream_t stream)
    {
        const size_t nTiles = (cap + BLOCK - 1) / BLOCK, nGroups = (nTiles + RESORT_GROUP - 1) / RESORT_GROUP;
        NRSCHK(wallList.alloc((size_t)cap * 4));
        NRSCHK(wallTile.alloc(nTiles * 4)); NRSCHK(wallTileOffset.alloc(nTiles * 4));
        NRSCHK(wallMask.alloc(nTiles * 4 * 8));
        NRSCHK(wallGroupTotal.alloc(nGroups * 4)); NRSCHK(wallGroupPrefix.alloc(nGroups * 4)); NRSCHK(wallScalars.alloc(16));
        HIPCHK(hipMemsetAsync(wallScalars.p, 0, 16, stream));
        return NRS_OK;
    }

    // ---- views -----------------------------------------------------------------------------------------------------------------------
    // nearBits: the boundary tables' bit per cell; hash: the sorted keys of the step
    WallList view(const uint32_t *nearBits, const uint32_t *hash) const
    {
        return WallList{nearBits, hash, wallList.as<uint32_t>(), wallScalars.as<uint32_t>() + 1, wallMask.as<unsigned long long>()};
    }
    uint32_t *tile_counts() const { return wallTile.as<uint32_t>(); }                  // per 256-slot tile: wall slots, counted by the reorder kernels
    unsigned long long *slot_masks() const { return wallMask.as<unsigned long long>(); } // ... which also mark them, a bit per slot

    // this step's wall list: tile counts (reorder kernel) -> two-level scan (the re-sort's scan kernel) -> stable compaction
    int build(uint32_t N, SortStage &sort, hipStream_t stream, const uint32_t *nearBits, const uint32_t *hash)
    {
        const uint32_t nTiles = nblocks(N);
        const WallList wl = view(nearBits, hash); // (the tile counts were left by the reorder kernel of this step)
        uint32_t *sc = wallScalars.as<uint32_t>();
        const ResortScan a = {wallTile.as<uint32_t>(), wallTileOffset.as<uint32_t>(), wallGroupTotal.as<uint32_t>(), wallGroupPrefix.as<uint32_t>(), sc + 1};
        NRSCHK(sort.scan_tiles(a, sc, nTiles));
        hipLaunchKernelGGL(k_wall_compact, dim3(nTiles), dim3(BLOCK), 0, stream, wl, wallTileOffset.as<uint32_t>(), wallGroupPrefix.as<uint32_t>(),
                           (uint32_t)RESORT_GROUP, wallList.as<uint32_t>(), N);
        HIPCHK(hipGetLastError());
        return NRS_OK;
    }

private:
    DevBuf wallList, wallTile, wallTileOffset, wallGroupTotal, wallGroupPrefix, wallScalars, wallMask;
};

} // namespace nrs
