// nrs_kernels_mesh.h — the device side of the mesh sampling (include/nereus_hip.h "mesh sampling" has the formulas; DESIGN.md "Mesh
// sampling" the reasons): the field kernel — one thread per lattice node, every triangle in ascending order — and the selection: selected
// nodes counted per workgroup, the totals scanned by one workgroup, the node indices (and snapped points) compacted in order, then
// turned into particles.  The rules are nrs_host_mesh.h's.  Double throughout, no atomics, no waiting between workgroups.
//
// The field kernel is bound by fp64 arithmetic (about 150 operations and one atan2 per pair), not by memory: the triangle index is the
// same in every lane, so the nine doubles of a triangle come through scalar loads from `tri` and cost no vector memory instruction and no
// LDS.  The triangles are walked MESH_UNROLL at a time so that the scalar loads of the next ones are in flight while one is evaluated.
#pragma once
#include <hip/hip_runtime.h>

#include "nrs_host_mesh.h"
#include "nrs_scan.h"

namespace nrs {

constexpr int MESH_BLOCK = 256;  // nodes per workgroup (4 waves)
constexpr int MESH_UNROLL = 4;   // triangles per trip of the field kernel's main loop; the rest go one at a time

struct MeshD3 { double x, y, z; };
__device__ __forceinline__ MeshD3 mesh_sub(MeshD3 a, MeshD3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double mesh_dot(MeshD3 a, MeshD3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ MeshD3 mesh_cross(MeshD3 a, MeshD3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// o + d * s per component
__device__ __forceinline__ MeshD3 mesh_along(MeshD3 o, MeshD3 d, double s) { return {o.x + d.x * s, o.y + d.y * s, o.z + d.z * s}; }

// node q of L (linear index) in double
__device__ __forceinline__ MeshD3 mesh_node(const Lattice &L, uint64_t q)
{
    const uint32_t i = (uint32_t)(q % L.dims[0]);
    const uint64_t t = q / L.dims[0];
    const uint32_t j = (uint32_t)(t % L.dims[1]), k = (uint32_t)(t / L.dims[1]);
    return {L.origin[0] + (double)i * L.spacing[0], L.origin[1] + (double)j * L.spacing[1], L.origin[2] + (double)k * L.spacing[2]};
}

// the running results of one node
struct MeshAcc {
    double acc;      // sum of 2 atan2
    double best;     // smallest squared distance so far
    MeshD3 q;        // its closest point
    uint32_t tri;    // its triangle
};

// one (node, triangle) pair
template <bool WIND, bool DIST>
__device__ __forceinline__ void mesh_pair(const double *__restrict__ T, uint32_t t, MeshD3 P, MeshAcc &R)
{
    const MeshD3 A = {T[0], T[1], T[2]}, B = {T[3], T[4], T[5]}, C = {T[6], T[7], T[8]};
    if (WIND) {
        const MeshD3 a = mesh_sub(A, P), b = mesh_sub(B, P), c = mesh_sub(C, P);
        const double la = sqrt(mesh_dot(a, a)), lb = sqrt(mesh_dot(b, b)), lc = sqrt(mesh_dot(c, c));
        const double num = mesh_dot(a, mesh_cross(b, c));
        const double den = la * lb * lc + mesh_dot(a, b) * lc + mesh_dot(b, c) * la + mesh_dot(c, a) * lb;
        R.acc += 2.0 * atan2(num, den);
    }
    if (DIST) {
        const MeshD3 ab = mesh_sub(B, A), ac = mesh_sub(C, A), ap = mesh_sub(P, A), bp = mesh_sub(P, B), cp = mesh_sub(P, C);
        const double d1 = mesh_dot(ab, ap), d2 = mesh_dot(ac, ap), d3 = mesh_dot(ab, bp), d4 = mesh_dot(ac, bp), d5 = mesh_dot(ab, cp),
                     d6 = mesh_dot(ac, cp);
        const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
        const double e43 = d4 - d3, e56 = d5 - d6;
        MeshD3 q;
        if (d1 <= 0.0 && d2 <= 0.0) q = A;
        else if (d3 >= 0.0 && d4 <= d3) q = B;
        else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) q = mesh_along(A, ab, d1 / (d1 - d3));
        else if (d6 >= 0.0 && d5 <= d6) q = C;
        else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) q = mesh_along(A, ac, d2 / (d2 - d6));
        else if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) q = mesh_along(B, mesh_sub(C, B), e43 / (e43 + e56));
        else {
            const double dn = 1.0 / (va + vb + vc);
            q = mesh_along(mesh_along(A, ab, vb * dn), ac, vc * dn);
        }
        const MeshD3 r = mesh_sub(P, q);
        const double dd = mesh_dot(r, r);
        if (dd < R.best) { R.best = dd; R.q = q; R.tri = t; }
    }
}

// where the field of a batch goes (device arrays of the batch's m nodes); null: not asked for
struct MeshFieldOut {
    double *w, *d2;
    uint32_t *tri;
    double *q; // 3 per node
};

// One thread per node first + i of L, i < m.  tri: 9 doubles per triangle (mesh_gather), nt of them.
// NRS_MESH_LDS_TILE (not defined in the library as shipped; tools/bench_mesh.py says how to build with it): the measured alternative,
// in which a workgroup stages that many triangles in LDS and every lane reads them from there by broadcast.
template <bool WIND, bool DIST>
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_field(Lattice L, uint64_t first, uint32_t m, const double *__restrict__ tri, uint32_t nt, MeshFieldOut O)
{
    const uint32_t i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    const bool live = i < m;
    const MeshD3 P = mesh_node(L, first + (live ? i : 0u));
    MeshAcc R;
    R.acc = 0.0; R.best = INFINITY; R.q = {0.0, 0.0, 0.0}; R.tri = 0xffffffffu;
#if defined(NRS_MESH_LDS_TILE)
    __shared__ double tile[9 * NRS_MESH_LDS_TILE];
    for (uint32_t t0 = 0; t0 < nt; t0 += NRS_MESH_LDS_TILE) {
        const uint32_t c = nt - t0 < (uint32_t)NRS_MESH_LDS_TILE ? nt - t0 : (uint32_t)NRS_MESH_LDS_TILE;
        __syncthreads(); // (the tile before this one has been read)
        for (uint32_t e = threadIdx.x; e < 9u * c; e += MESH_BLOCK) tile[e] = tri[9 * (size_t)t0 + e];
        __syncthreads();
        if (live)
            for (uint32_t u = 0; u < c; ++u) mesh_pair<WIND, DIST>(tile + 9 * u, t0 + u, P, R);
    }
    if (!live) return;
#else
    if (!live) return;
    uint32_t t = 0;
    for (; t + MESH_UNROLL <= nt; t += MESH_UNROLL) {
#pragma unroll
        for (int u = 0; u < MESH_UNROLL; ++u) mesh_pair<WIND, DIST>(tri + 9 * (size_t)(t + u), t + u, P, R);
    }
    for (; t < nt; ++t) mesh_pair<WIND, DIST>(tri + 9 * (size_t)t, t, P, R);
#endif
    if (WIND && O.w) O.w[i] = R.acc / (4.0 * 3.14159265358979323846);
    if (DIST) {
        if (O.d2) O.d2[i] = R.best;
        if (O.tri) O.tri[i] = R.tri;
        if (O.q) { O.q[3 * (size_t)i] = R.q.x; O.q[3 * (size_t)i + 1] = R.q.y; O.q[3 * (size_t)i + 2] = R.q.z; }
    }
}

// ---- the selection ---------------------------------------------------------------------------------------------------------------------------
// total: the selected nodes of the batches so far; base: those before the batch whose scan ran last
struct MeshHeader {
    uint32_t total, base;
    uint32_t pad[2];
};
__device__ __forceinline__ bool mesh_keep(const MeshSelect &S, const double *__restrict__ w, const double *__restrict__ d2, uint32_t i)
{
    return mesh_selected(S, S.useW ? w[i] : 0.0, S.useD ? d2[i] : 0.0);
}
// 1. the selected nodes per workgroup
static __global__ __launch_bounds__(MESH_BLOCK) void k_mesh_count(MeshSelect S, const double *__restrict__ w, const double *__restrict__ d2, uint32_t m,
                                                                  uint32_t *__restrict__ blockTot)
{
    __shared__ uint32_t wsum[MESH_BLOCK / 64];
    const uint32_t i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    const bool keep = i < m && mesh_keep(S, w, d2, i);
    const uint32_t c = (uint32_t)__popcll(__ballot(keep));
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
#pragma unroll
        for (uint32_t v = 0; v < MESH_BLOCK / 64; ++v) all += wsum[v];
        blockTot[blockIdx.x] = all;
    }
}
// 2. one workgroup: the exclusive scan of the totals in place; the header moves on by the batch's total
static __global__ __launch_bounds__(SCAN_BLOCK) void k_mesh_scan(uint32_t *__restrict__ blockTot, uint32_t nb, MeshHeader *__restrict__ hdr)
{
    __shared__ uint32_t wsum[SCAN_BLOCK / 64];
    const uint32_t S = scan_list(blockTot, nb, wsum);
    if (threadIdx.x == 0) {
        const uint32_t before = hdr->total;
        hdr->base = before;
        hdr->total = before + S;
    }
}
// 3. the selected nodes of the batch, in order, behind those of the batches before: the node's linear index and, unless selQ is
// null, its closest point.  Slots at or above `limit` are not written (the caller learns from the total that they did not fit).
static __global__ __launch_bounds__(MESH_BLOCK) void k_mesh_compact(MeshSelect S, const double *__restrict__ w, const double *__restrict__ d2,
                                                                    const double *__restrict__ q, uint64_t first, uint32_t m,
                                                                    const uint32_t *__restrict__ blockOff, const MeshHeader *__restrict__ hdr,
                                                                    uint64_t limit, uint32_t *__restrict__ selIdx, double *__restrict__ selQ)
{
    __shared__ uint32_t wsum[MESH_BLOCK / 64];
    const uint32_t i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    const uint32_t keep = (i < m && mesh_keep(S, w, d2, i)) ? 1u : 0u;
    const uint64_t to = (uint64_t)hdr->base + blockOff[blockIdx.x] + block_scan<MESH_BLOCK>(keep, wsum);
    if (!keep || to >= limit) return;
    selIdx[to] = (uint32_t)(first + i); // (a lattice has at most 2^31 nodes)
    if (selQ) {
        selQ[3 * to] = q[3 * (size_t)i];
        selQ[3 * to + 1] = q[3 * (size_t)i + 1];
        selQ[3 * to + 2] = q[3 * (size_t)i + 2];
    }
}
// 4. nrs_mesh_particles: selected node s as an SVec4, one rounding per component
template <typename T4, typename R>
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_positions(Lattice L, const uint32_t *__restrict__ selIdx, const double *__restrict__ selQ, uint32_t count,
                                                               T4 *__restrict__ pos)
{
    const uint32_t s = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (s >= count) return;
    MeshD3 x;
    if (selQ) x = {selQ[3 * (size_t)s], selQ[3 * (size_t)s + 1], selQ[3 * (size_t)s + 2]};
    else x = mesh_node(L, selIdx[s]);
    T4 p;
    p.x = (R)x.x; p.y = (R)x.y; p.z = (R)x.z; p.w = (R)1;
    pos[s] = p;
}

} // namespace nrs
