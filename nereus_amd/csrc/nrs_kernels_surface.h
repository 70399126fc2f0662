// nrs_kernels_surface.h — marching tetrahedra on the sampler's lattice (include/nereus_hip.h "surface extraction"; DESIGN.md "Surface
// extraction").  The rules — corners, edges, tetrahedra, cases, the per-node and per-cell routines — are nrs_host_surface.h's; here are
// the four launches that apply them, one thread per node with x fastest (a node is also the low corner of "its" cell):
//   k_surf_count      per node the vertex count (0..7) and its cell's triangle count (0..12), reduced to one pair per workgroup
//   k_surf_scan       one workgroup: exclusive scan of the pairs; the element behind the last is (V, T)
//   k_surf_vertices   the count again, a workgroup-local exclusive scan on top of the workgroup's offset: the node's vertex offset and
//                     edge mask are stored, the vertex records and attributes written
//   k_surf_triangles  the same for the triangles; vertex number of (corner node n, edge e) = offset[n] + popcount(mask[n] & ((1 << e) - 1))
// The order of every output is the order of the scan: no atomics.  The kernels depend on the real type only.
#pragma once
#include <hip/hip_runtime.h>

#include "nrs_host_surface.h"
#include "nrs_scan.h"

namespace nrs {

constexpr int SURF_BLOCK = 256; // nodes per workgroup of the three lattice kernels (4 waves)

template <typename R> struct SurfVec4;
template <> struct SurfVec4<float> { typedef float4 type; };
template <> struct SurfVec4<double> { typedef double4 type; };

// node q of the lattice: indices, which + neighbours exist, and the eight densities of its cell's corners (only the existing ones are read)
struct SurfNodeIdx { uint32_t i, j, k, have; };
__device__ __forceinline__ SurfNodeIdx surf_node_idx(const Lattice &L, uint32_t q)
{
    SurfNodeIdx n;
    n.i = q % L.dims[0];
    const uint32_t t = q / L.dims[0];
    n.j = t % L.dims[1];
    n.k = t / L.dims[1];
    n.have = surf_have(L, n.i, n.j, n.k);
    return n;
}
// linear offset of the node at direction code d from a node
__device__ __forceinline__ uint32_t surf_dir_offset(const Lattice &L, uint32_t d)
{
    return (d & 1u) + ((d >> 1) & 1u) * L.dims[0] + ((d >> 2) & 1u) * L.dims[0] * L.dims[1];
}
template <typename R> __device__ __forceinline__ void surf_load(const R *__restrict__ dens, const Lattice &L, uint32_t q, uint32_t have, R f[8])
{
#pragma unroll
    for (uint32_t d = 0; d < 8; ++d) f[d] = (d & ~have) ? (R)0 : dens[q + surf_dir_offset(L, d)];
}

// ---- 1. mark and reduce ---------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ __launch_bounds__(SURF_BLOCK) void k_surf_count(const R *__restrict__ dens, Lattice L, R iso, uint32_t nodes, uint2 *__restrict__ blockTot)
{
    __shared__ uint32_t wsum[SURF_BLOCK / 64];
    const uint32_t q = blockIdx.x * SURF_BLOCK + threadIdx.x;
    uint32_t packed = 0; // vertices | triangles << 16: a workgroup has at most 7 * 256 and 12 * 256
    if (q < nodes) {
        const SurfNodeIdx n = surf_node_idx(L, q);
        R f[8];
        surf_load<R>(dens, L, q, n.have, f);
        const uint32_t bits = surf_inside_bits<R>(f, iso, n.have);
        packed = surf_popcount(surf_node_mask(bits, n.have));
        if (n.have == 7u) packed |= surf_cell_count(bits) << 16;
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) packed += (uint32_t)__shfl_down((int)packed, d, 64);
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = packed;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t i = 0; i < SURF_BLOCK / 64; ++i) s += wsum[i];
        blockTot[blockIdx.x] = make_uint2(s & 0xffffu, s >> 16);
    }
}

// ---- 2. exclusive scan of the nb workgroup totals, in place; tot[nb] = (V, T) ------------------------------------------------------------------
__global__ __launch_bounds__(SCAN_BLOCK) void k_surf_scan(uint2 *__restrict__ tot, uint32_t nb)
{
    __shared__ uint2 wsum[SCAN_BLOCK / 64];
    const uint2 all = scan_list(tot, nb, wsum);
    if (threadIdx.x == 0) tot[nb] = all;
}

// ---- 3. vertex emit -------------------------------------------------------------------------------------------------------------------------------
template <typename R> struct SurfVertexOut {
    typedef typename SurfVec4<R>::type T4;
    uint32_t *nodeOff; // per node: the number of its first vertex
    uint8_t *nodeMask; // per node: its edge mask
    T4 *vert, *grad, *vel; // V records each; grad / vel null: not asked for
};
template <typename T4, typename R> __device__ __forceinline__ T4 surf_lerp4(const T4 &a, const T4 &b, R t)
{
    T4 r;
    r.x = surf_lerp<R>(a.x, b.x, t); r.y = surf_lerp<R>(a.y, b.y, t); r.z = surf_lerp<R>(a.z, b.z, t); r.w = surf_lerp<R>(a.w, b.w, t);
    return r;
}
template <typename R>
__global__ __launch_bounds__(SURF_BLOCK) void k_surf_vertices(const R *__restrict__ dens, const typename SurfVec4<R>::type *__restrict__ sGrad,
                                                              const typename SurfVec4<R>::type *__restrict__ sVel, Lattice L, R iso, uint32_t nodes,
                                                              const uint2 *__restrict__ blockOff, SurfVertexOut<R> O)
{
    typedef typename SurfVec4<R>::type T4;
    __shared__ uint32_t wsum[SURF_BLOCK / 64];
    const uint32_t q = blockIdx.x * SURF_BLOCK + threadIdx.x;
    const bool live = q < nodes;
    SurfNodeIdx n = {0u, 0u, 0u, 0u};
    R f[8];
    uint32_t mask = 0;
    if (live) {
        n = surf_node_idx(L, q);
        surf_load<R>(dens, L, q, n.have, f);
        mask = surf_node_mask(surf_inside_bits<R>(f, iso, n.have), n.have);
    }
    const uint32_t first = blockOff[blockIdx.x].x + block_scan<SURF_BLOCK>(surf_popcount(mask), wsum);
    if (!live) return;
    O.nodeOff[q] = first;
    O.nodeMask[q] = (uint8_t)mask;
    if (!mask) return;
    const R p0x = surf_node_coord<R>(L, 0, n.i), p0y = surf_node_coord<R>(L, 1, n.j), p0z = surf_node_coord<R>(L, 2, n.k);
    const R p1x = surf_node_coord<R>(L, 0, n.i + 1u), p1y = surf_node_coord<R>(L, 1, n.j + 1u), p1z = surf_node_coord<R>(L, 2, n.k + 1u);
    uint32_t v = first;
#pragma unroll
    for (uint32_t e = 0; e < 7; ++e) {
        if (!((mask >> e) & 1u)) continue;
        const uint32_t d = surf_edge_dir(e);
        const R t = surf_vertex_t<R>(iso, f[0], f[d]);
        T4 x;
        x.x = surf_lerp<R>(p0x, (d & 1u) ? p1x : p0x, t);
        x.y = surf_lerp<R>(p0y, (d & 2u) ? p1y : p0y, t);
        x.z = surf_lerp<R>(p0z, (d & 4u) ? p1z : p0z, t);
        x.w = t;
        O.vert[v] = x;
        const uint32_t far = q + surf_dir_offset(L, d);
        if (O.grad) O.grad[v] = surf_lerp4<T4, R>(sGrad[q], sGrad[far], t);
        if (O.vel) O.vel[v] = surf_lerp4<T4, R>(sVel[q], sVel[far], t);
        ++v;
    }
}

// ---- 4. triangle emit ---------------------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ __launch_bounds__(SURF_BLOCK) void k_surf_triangles(const R *__restrict__ dens, Lattice L, R iso, uint32_t nodes, const uint2 *__restrict__ blockOff,
                                                               const uint32_t *__restrict__ nodeOff, const uint8_t *__restrict__ nodeMask, uint32_t *__restrict__ tri)
{
    __shared__ uint32_t wsum[SURF_BLOCK / 64];
    const uint32_t q = blockIdx.x * SURF_BLOCK + threadIdx.x;
    uint32_t bits = 0, count = 0;
    if (q < nodes) {
        const SurfNodeIdx n = surf_node_idx(L, q);
        if (n.have == 7u) {
            R f[8];
            surf_load<R>(dens, L, q, 7u, f);
            bits = surf_inside_bits<R>(f, iso, 7u);
            count = surf_cell_count(bits);
        }
    }
    const uint32_t first = blockOff[blockIdx.x].y + block_scan<SURF_BLOCK>(count, wsum);
    if (!count) return;
    // the vertex offsets and masks of the cell's eight corner nodes; corner 7 owns no edge of this cell
    uint32_t off[7], msk[7];
#pragma unroll
    for (uint32_t c = 0; c < 7; ++c) {
        const uint32_t nq = q + surf_dir_offset(L, c);
        off[c] = nodeOff[nq];
        msk[c] = nodeMask[nq];
    }
    surf_cell_triangles(bits, [&](uint32_t k, uint32_t c0, uint32_t e0, uint32_t c1, uint32_t e1, uint32_t c2, uint32_t e2) {
        uint32_t *o = tri + 3u * (size_t)(first + k);
        const uint32_t cs[3] = {c0, c1, c2}, es[3] = {e0, e1, e2};
#pragma unroll
        for (uint32_t i = 0; i < 3; ++i) {
            uint32_t base = 0, m = 0;
#pragma unroll
            for (uint32_t c = 0; c < 7; ++c)
                if (cs[i] == c) { base = off[c]; m = msk[c]; }
            o[i] = base + surf_popcount(m & ((1u << es[i]) - 1u));
        }
    });
}

} // namespace nrs
