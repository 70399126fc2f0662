// nrs_kernels_inflow.h — the device side of the sources and sinks (include/nereus_hip.h "sources and sinks"; DESIGN.md "Sources and
// sinks"): the sites of emitted layers, of a lattice block and of a mesh selection (nrs_emit_mesh) written behind the living
// particles, and the cull — survivors counted per workgroup, the totals scanned by one workgroup, the arrays compacted in order.  The rules (frame, sites, predicate) are
// nrs_host_inflow.h's; the host schedules, so no kernel here decides how many particles there are.  No atomics, no waiting between
// workgroups: every offset comes from a scan, every output is bit-reproducible.
#pragma once
#include "nrs_host_inflow.h"
#include "nrs_kernels_sample.h" // lattice_node
#include "nrs_scan.h"

namespace nrs {

// what the cull leaves for the host
struct InflowHeader {
    uint32_t survivors; // of the last count
    uint32_t pad[3];
};

// ---- emission ------------------------------------------------------------------------------------------------------------------------------
// `layers` layers of one emitter (origins o[l]) of `sites` sites each; disc: the rows' half widths and starts (InflowSites)
struct EmitArgs {
    double o[INFLOW_LAYERS_PER_LAUNCH][3];
    double e1[3], e2[3], s;
    double v[3]; // speed * d
    uint32_t layers, sites, ku, kv, disc;
};
// the arrays a new particle is written to (kv: DFSPH only, else null), from slot `first` on; with particle tracking (nrs_track.h) also its
// id = firstId + t for the launch's site t, its birth stamp and (rec: null without the attribute record) the slot's emit value
template <typename R> struct EmitOut {
    typedef typename Vec4T<R>::type T4;
    T4 *pos, *vel;
    R *pres, *kv;
    uint32_t first;
    uint32_t *id, *birth; // null: the context does not track
    T4 *rec;
    uint32_t firstId, birthNow;
    T4 recValue;
};
template <typename R> NRS_DEV void emit_store(const EmitOut<R> &O, uint32_t t, R x, R y, R z, R vx, R vy, R vz)
{
    const uint32_t to = O.first + t;
    O.pos[to] = mk4<R>(x, y, z, (R)1);
    O.vel[to] = mk4<R>(vx, vy, vz, (R)0);
    O.pres[to] = (R)0;
    if (O.kv) O.kv[to] = (R)0;
    if (O.id) {
        O.id[to] = O.firstId + t;
        O.birth[to] = O.birthNow;
        if (O.rec) O.rec[to] = O.recValue;
    }
}
// One thread per (layer, site), layer-major; which (i, j) site k is and where it lies: inflow_site, inflow_site_pos (nrs_host_inflow.h)
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_inflow_emit(EmitArgs A, const int32_t *__restrict__ rowHalf, const uint32_t *__restrict__ rowStart, EmitOut<R> O)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= A.layers * A.sites) return;
    const uint32_t l = t / A.sites, k = t - l * A.sites;
    int32_t i, j;
    inflow_site(k, A.ku, A.kv, A.disc != 0u, rowHalf, rowStart, i, j);
    R x[3];
    inflow_site_pos<R>(A.o[l], A.e1, A.e2, A.s, i, j, x);
    emit_store<R>(O, t, x[0], x[1], x[2], (R)A.v[0], (R)A.v[1], (R)A.v[2]);
}
// nrs_emit_block: one thread per node of L in its linear index order
template <typename R> __global__ __launch_bounds__(BLOCK) void k_inflow_block(Lattice L, double vx, double vy, double vz, uint32_t m, EmitOut<R> O)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= m) return;
    const uint32_t i = q % L.dims[0], t = q / L.dims[0];
    const V3<R> x = lattice_node<R>(L, i, t % L.dims[1], t / L.dims[1]);
    emit_store<R>(O, q, x.x, x.y, x.z, (R)vx, (R)vy, (R)vz);
}
// nrs_emit_mesh: one thread per selected node; sel[t] is its linear index in L (ascending: the selection keeps the lattice's order)
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_inflow_sites(Lattice L, const uint32_t *__restrict__ sel, double vx, double vy, double vz, uint32_t m, EmitOut<R> O)
{
    const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
    if (s >= m) return;
    const uint32_t q = sel[s];
    const uint32_t i = q % L.dims[0], t = q / L.dims[0];
    const V3<R> x = lattice_node<R>(L, i, t % L.dims[1], t / L.dims[1]);
    emit_store<R>(O, s, x.x, x.y, x.z, (R)vx, (R)vy, (R)vz);
}

// ---- the cull ----------------------------------------------------------------------------------------------------------------------------------
// 1. survivors per workgroup: the predicate, a ballot per wave, its population count, the sum over the workgroup's waves
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_cull_count(const typename Vec4T<R>::type *__restrict__ pos, CullBounds<R> B, uint32_t n, uint32_t *__restrict__ blockTot)
{
    __shared__ uint32_t wsum[BLOCK / 64];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    bool keep = false;
    if (i < n) {
        const typename Vec4T<R>::type p = pos[i];
        keep = !inflow_caught<R>(B, p.x, p.y, p.z);
    }
    const uint32_t c = (uint32_t)__popcll(__ballot(keep));
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
#pragma unroll
        for (uint32_t w = 0; w < BLOCK / 64; ++w) all += wsum[w];
        blockTot[blockIdx.x] = all;
    }
}
// 2. one workgroup: the exclusive scan of the totals in place, the survivor count into the header
static __global__ __launch_bounds__(SCAN_BLOCK) void k_cull_scan(uint32_t *__restrict__ blockTot, uint32_t nb, InflowHeader *__restrict__ hdr)
{
    __shared__ uint32_t wsum[SCAN_BLOCK / 64];
    const uint32_t S = scan_list(blockTot, nb, wsum);
    if (threadIdx.x == 0) hdr->survivors = S;
}
// 3. the survivors move, in order: the predicate again, a scan inside the workgroup, the workgroup's offset from the scanned totals
template <typename R> struct CullArrays {
    typedef typename Vec4T<R>::type T4;
    const T4 *pos, *vel;
    const R *pres, *kv; // kv: DFSPH only, else null
    T4 *posTo, *velTo;
    R *presTo, *kvTo;
    // particle tracking (nrs_track.h): id null when the context does not track, rec null without the attribute record
    const uint32_t *id, *birth;
    const T4 *rec;
    uint32_t *idTo, *birthTo;
    T4 *recTo;
};
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_cull_compact(CullArrays<R> A, CullBounds<R> B, uint32_t n, const uint32_t *__restrict__ blockOff)
{
    __shared__ uint32_t wsum[BLOCK / 64];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    typename Vec4T<R>::type p = {};
    uint32_t keep = 0;
    if (i < n) {
        p = A.pos[i];
        keep = inflow_caught<R>(B, p.x, p.y, p.z) ? 0u : 1u;
    }
    const uint32_t to = blockOff[blockIdx.x] + block_scan<BLOCK>(keep, wsum);
    if (!keep) return;
    A.posTo[to] = p; // (to <= i < n)
    A.velTo[to] = A.vel[i];
    A.presTo[to] = A.pres[i];
    if (A.kv) A.kvTo[to] = A.kv[i];
    if (A.id) {
        A.idTo[to] = A.id[i];
        A.birthTo[to] = A.birth[i];
        if (A.rec) A.recTo[to] = A.rec[i];
    }
}

} // namespace nrs
