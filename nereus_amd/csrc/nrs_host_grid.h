// nrs_host_grid.h — the rule that makes a grid from the boundary particles' bounding box (nrs_set_boundaries with update_grid;
// BBMin / BBMax sph/sph_cuda.cu:461-505 + SPH::updateGrid sph/sph.cpp:313-337), and the key width of the (hash, index) sorts.  No HIP.
// R is the context's SReal; every expression is evaluated in the types the reference evaluates it in: SReal promoted to double where a
// double literal meets it, rounded to SReal where it is stored.
#pragma once
#include <cmath>
#include <cstdint>

#include "nrs_error.h"

namespace nrs {

static inline uint32_t next_pow2(uint32_t v) // sph/sph.cpp:300-311
{
    v--;
    v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16;
    v++;
    return v;
}

// bits of a cell hash: what the radix sorts of the fluid's and of the boundary's pairs are told to look at
static inline uint32_t sort_key_bits(uint32_t numCells)
{
    uint32_t bits = 1;
    while (bits < 32 && (1ull << bits) < (uint64_t)numCells) ++bits;
    return bits;
}

// the bounding box of n >= 1 points (x, y, z, w) in SReal
template <typename R> static inline void aabb_of_points(const R *p4, uint64_t n, R mn[3], R mx[3])
{
    for (int a = 0; a < 3; ++a) mn[a] = mx[a] = p4[a];
    for (uint64_t i = 1; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const R c = p4[4 * i + a];
            if (c < mn[a]) mn[a] = c;
            if (mx[a] < c) mx[a] = c;
        }
}

template <typename R> struct AabbGrid {
    R origin[3];
    uint32_t size[3];
    uint32_t numCells;
};
// origin = min - 0.1, extent = next_pow2(ceil((max - min + 0.1) / h)) per axis; refused beyond 2^31 cells, g untouched then
template <typename R> static inline int grid_from_aabb(const R mn[3], const R mx[3], R h, AabbGrid<R> &g)
{
    AabbGrid<R> o;
    for (int a = 0; a < 3; ++a) {
        o.origin[a] = (R)(mn[a] - 0.1);
        const uint32_t sz = (uint32_t)std::ceil((mx[a] - mn[a] + 0.1) / h);
        o.size[a] = next_pow2(sz);
    }
    const uint64_t C = (uint64_t)o.size[0] * o.size[1] * o.size[2];
    if (C > (1ull << 31)) return fail(NRS_E_INVALID, "grid from boundary AABB exceeds 2^31 cells");
    o.numCells = (uint32_t)C;
    g = o;
    return NRS_OK;
}

} // namespace nrs
