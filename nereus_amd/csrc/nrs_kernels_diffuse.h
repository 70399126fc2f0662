// nrs_kernels_diffuse.h — the launches of one nrs_diffuse_step (include/nereus_hip.h "diffuse particles"; DESIGN.md "Diffuse
// particles").  The per-particle rules — hash, clamp, birth count, birth, advection — are nrs_host_diffuse.h's; the neighbour walk at a
// diffuse particle is the sampler's sample_walk.  After the sampler's gather has written the density gradients of the sorted fluid:
//   k_diffuse_potentials  per sorted fluid particle: the three potentials, the rate, the births and the parent's kind; births reduced
//                         to one total per workgroup
//   k_diffuse_advect      per diffuse slot below the capacity: the new state into the staging arrays and a survivor flag (0 beyond the
//                         living count); flags reduced to one total per workgroup
//   k_diffuse_scan        one workgroup: exclusive scans of both lists of totals; the header gets the survivors S, the new living
//                         count min(S + B, capacity) and the births dropped
//   k_diffuse_compact     the flags again, a workgroup-local exclusive scan on top of the workgroup's offset: survivors move from the
//                         staging arrays to the front of the set, in their order
//   k_diffuse_births      the same over the births: birth k of slot i goes to S + offset_i + k if that is below the capacity
// The order of every output is the order of a scan: no atomics.  The living count never leaves the device.
#pragma once
#include "nrs_host_diffuse.h"
#include "nrs_kernels_sample.h"
#include "nrs_scan.h"

namespace nrs {

// the counters of a diffuse set on the device
struct DiffuseHeader {
    uint32_t alive;     // living particles
    uint32_t survivors; // of the last step: where its births start
    uint64_t dropped;   // births refused for capacity since configure
    uint32_t byKind[3]; // filled by k_diffuse_kinds for nrs_diffuse_count
    uint32_t pad;
};

template <typename R> NRS_DEV D3<R> d3(V3<R> a) { D3<R> d; d.x = a.x; d.y = a.y; d.z = a.z; return d; }

// ---- 1. potentials and births per sorted fluid particle ---------------------------------------------------------------------------------
template <typename R> struct DiffuseFluidOut {
    typedef typename Vec4T<R>::type T4;
    T4 *potentials;       // (I_ta, I_wc, I_k, rate)
    uint32_t *births;
    uint32_t *parentKind; // the kind a birth of this particle gets
    uint32_t *blockTot;   // births per workgroup
};
template <typename R, int KSET>
__global__ __launch_bounds__(BLOCK) void k_diffuse_potentials(Params<R> P, GridView<R> G, const typename Vec4T<R>::type *__restrict__ sPos,
                                                              const typename Vec4T<R>::type *__restrict__ sVel,
                                                              const typename Vec4T<R>::type *__restrict__ grad, DiffuseCfg<R> C, uint64_t step, R dt,
                                                              DiffuseFluidOut<R> O, uint32_t n)
{
    __shared__ uint32_t wsum[BLOCK / 64];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t births = 0;
    if (i < n) {
        const R ir = P.interactionRadius;
        const V3<R> xi = xyz<R>(sPos[i]), vi = xyz<R>(sVel[i]), gi = xyz<R>(grad[i]);
        // the outward unit normal and the gate of the wave crest
        const float gl = length(gi);
        V3<R> ni = mk3<R>(0, 0, 0);
        bool crest = false;
        if (gl != 0.0f) {
            const R l = (R)gl;
            ni = mk3<R>(-gi.x / l, -gi.y / l, -gi.z / l);
            const float vl = length(vi);
            if (vl != 0.0f) crest = (vi.x * ni.x + vi.y * ni.y + vi.z * ni.z) / (R)vl >= (R)0.6;
        }
        R ta = (R)0, wc = (R)0;
        uint32_t cnt = 1u; // the particle itself: what sample_walk counts at x_i
        bool finite = finite3<R>(xi);
        if (finite) {
            const I3 gp = calcGridPos<R>(P, xi);
            for (int z = -1; z <= 1; z++)
                for (int y = -1; y <= 1; y++)
                    for (int c = -1; c <= 1; c++) {
                        const uint32_t h = calcGridHash<R>(P, (int)((uint32_t)gp.x + (uint32_t)c), (int)((uint32_t)gp.y + (uint32_t)y), (int)((uint32_t)gp.z + (uint32_t)z));
                        const uint32_t s = G.cellStart[h];
                        if (s == CELL_EMPTY) continue;
                        const uint32_t e = G.cellEnd[h];
                        if (!run_ok<R>(G, s, e)) continue;
                        for (uint32_t j = s; j < e; ++j) {
                            if (j == i) continue;
                            const V3<R> xij = xi - xyz<R>(sPos[j]);
                            const float len = length(xij);
                            if (!(len < ir)) continue;
                            ++cnt;
                            const R r = (R)len;
                            const R wl = (R)1 - r / ir;
                            if (len != 0.0f) {
                                const V3<R> vij = vi - xyz<R>(sVel[j]);
                                const float vl = length(vij);
                                if (vl != 0.0f) {
                                    const R lv = (R)vl;
                                    const R cs = (vij.x * xij.x + vij.y * xij.y + vij.z * xij.z) / (lv * r);
                                    const R om = (R)1 - cs; // (float lengths in an fp64 build: the cosine may pass 1 by a float ulp)
                                    ta += lv * (om > (R)0 ? om : (R)0) * wl;
                                }
                                if (crest && (xij.x * ni.x + xij.y * ni.y + xij.z * ni.z) > (R)0) {
                                    const V3<R> gj = xyz<R>(grad[j]);
                                    const float gjl = length(gj);
                                    if (gjl != 0.0f) {
                                        const R l = (R)gjl;
                                        const V3<R> nj = mk3<R>(-gj.x / l, -gj.y / l, -gj.z / l);
                                        const R om = (R)1 - (ni.x * nj.x + ni.y * nj.y + ni.z * nj.z);
                                        wc += (om > (R)0 ? om : (R)0) * wl;
                                    }
                                }
                            }
                        }
                    }
        }
        const R ek = ((R)0.5 * P.particleMass) * (vi.x * vi.x + vi.y * vi.y + vi.z * vi.z);
        const R ita = diffuse_clamp<R>(ta, C.taMin, C.taMax), iwc = diffuse_clamp<R>(wc, C.wcMin, C.wcMax), ik = diffuse_clamp<R>(ek, C.kMin, C.kMax);
        const R rate = diffuse_rate<R>(C, ita, iwc, ik);
        births = finite ? diffuse_births<R>(C, rate, dt, diffuse_uniform<R>(C.seed, step, i, 0u)) : 0u;
        O.potentials[i] = mk4<R>(ita, iwc, ik, rate);
        O.births[i] = births;
        O.parentKind[i] = diffuse_kind(cnt, C.sprayBelow, C.bubbleAbove);
    }
    uint32_t total;
    block_scan<BLOCK>(births, wsum, &total);
    if (threadIdx.x == 0) O.blockTot[blockIdx.x] = total;
}

// ---- 2. advection of the living set ---------------------------------------------------------------------------------------------------------
template <typename R> struct DiffuseSet {
    typedef typename Vec4T<R>::type T4;
    T4 *pos, *vel;
    uint32_t *kind;
};
template <typename R, int KSET>
__global__ __launch_bounds__(BLOCK) void k_diffuse_advect(Params<R> P, GridView<R> G, const typename Vec4T<R>::type *__restrict__ sPos,
                                                          const typename Vec4T<R>::type *__restrict__ sVel, DiffuseCfg<R> C, R dt,
                                                          const DiffuseHeader *__restrict__ hdr, DiffuseSet<R> cur, DiffuseSet<R> staged,
                                                          uint32_t *__restrict__ flag, uint32_t *__restrict__ blockTot)
{
    __shared__ uint32_t wsum[BLOCK / 64];
    const uint32_t d = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t keep = 0;
    if (d < C.capacity) {
        if (d < hdr->alive) {
            const typename Vec4T<R>::type p4 = cur.pos[d];
            const V3<R> x = xyz<R>(p4), v = xyz<R>(cur.vel[d]);
            if (finite3<R>(x)) {
                SampleAcc<R> A = sample_acc_zero<R>();
                if (G.nSorted) A = sample_walk<R, KSET, false>(P, G, sPos, sVel, x, NRS_FIELD_VELOCITY);
                D3<R> vt = {(R)0, (R)0, (R)0};
                if (A.wsum != (R)0) { vt.x = A.vnum.x / A.wsum; vt.y = A.vnum.y / A.wsum; vt.z = A.vnum.z / A.wsum; }
                const D3<R> g = {P.gravity[0], P.gravity[1], P.gravity[2]};
                const D3<R> lo = {P.worldOrigin[0], P.worldOrigin[1], P.worldOrigin[2]};
                const D3<R> hi = {P.worldOrigin[0] + (R)P.gridSize[0] * P.cellSize[0], P.worldOrigin[1] + (R)P.gridSize[1] * P.cellSize[1],
                                  P.worldOrigin[2] + (R)P.gridSize[2] * P.cellSize[2]};
                const DiffuseState<R> s = diffuse_advect<R>(C, d3<R>(x), d3<R>(v), p4.w, vt, A.count, g, dt, lo, hi);
                if (s.alive) {
                    keep = 1u;
                    staged.pos[d] = mk4<R>(s.x.x, s.x.y, s.x.z, s.life);
                    staged.vel[d] = mk4<R>(s.v.x, s.v.y, s.v.z, (R)0);
                    staged.kind[d] = s.kind;
                }
            }
        }
        flag[d] = keep;
    }
    uint32_t total;
    block_scan<BLOCK>(keep, wsum, &total);
    if (threadIdx.x == 0) blockTot[blockIdx.x] = total;
}

// ---- 3. both scans and the header --------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(SCAN_BLOCK) void k_diffuse_scan(uint32_t *__restrict__ keepTot, uint32_t nbKeep, uint32_t *__restrict__ birthTot,
                                                                  uint32_t nbBirth, uint32_t capacity, DiffuseHeader *__restrict__ hdr)
{
    __shared__ uint32_t wsum[SCAN_BLOCK / 64];
    const uint32_t S = scan_list(keepTot, nbKeep, wsum);
    const uint32_t B = scan_list(birthTot, nbBirth, wsum);
    if (threadIdx.x == 0) {
        const uint64_t all = (uint64_t)S + B;
        const uint32_t alive = all < capacity ? (uint32_t)all : capacity;
        hdr->survivors = S;
        hdr->alive = alive;
        hdr->dropped += all - alive;
    }
}

// ---- 4. survivors to the front -------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_diffuse_compact(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ blockOff, DiffuseSet<R> staged,
                                                           DiffuseSet<R> cur, uint32_t capacity)
{
    __shared__ uint32_t wsum[BLOCK / 64];
    const uint32_t d = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t keep = d < capacity ? flag[d] : 0u;
    const uint32_t to = blockOff[blockIdx.x] + block_scan<BLOCK>(keep, wsum);
    if (!keep) return;
    cur.pos[to] = staged.pos[d]; // (to <= d: the staging arrays are read, the set is written)
    cur.vel[to] = staged.vel[d];
    cur.kind[to] = staged.kind[d];
}

// ---- 5. births behind them ---------------------------------------------------------------------------------------------------------------------------
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_diffuse_births(Params<R> P, const typename Vec4T<R>::type *__restrict__ sPos,
                                                          const typename Vec4T<R>::type *__restrict__ sVel, DiffuseCfg<R> C, uint64_t step, R dt,
                                                          const uint32_t *__restrict__ births, const uint32_t *__restrict__ parentKind,
                                                          const uint32_t *__restrict__ blockOff, const DiffuseHeader *__restrict__ hdr, DiffuseSet<R> cur,
                                                          uint32_t n)
{
    __shared__ uint32_t wsum[BLOCK / 64];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t b = i < n ? births[i] : 0u;
    const uint64_t first = (uint64_t)hdr->survivors + blockOff[blockIdx.x] + block_scan<BLOCK>(b, wsum);
    if (!b || first >= C.capacity) return;
    const D3<R> xi = d3<R>(xyz<R>(sPos[i])), vi = d3<R>(xyz<R>(sVel[i]));
    const uint32_t kind = parentKind[i];
    for (uint32_t k = 0; k < b && first + k < C.capacity; ++k) {
        const DiffuseBirth<R> nb = diffuse_birth<R>(C, step, i, k, xi, vi, P.particleRadius, dt);
        const uint32_t to = (uint32_t)(first + k);
        cur.pos[to] = mk4<R>(nb.x.x, nb.x.y, nb.x.z, nb.life);
        cur.vel[to] = mk4<R>(nb.v.x, nb.v.y, nb.v.z, (R)0);
        cur.kind[to] = kind;
    }
}

// ---- the header from the host's side: set the living count (upload, a changed capacity), restart `dropped` (configure) -----------------------
static __global__ void k_diffuse_header(DiffuseHeader *hdr, uint32_t alive, int setAlive, int clearDropped)
{
    if (threadIdx.x || blockIdx.x) return;
    if (setAlive) { hdr->alive = alive; hdr->survivors = alive; }
    if (clearDropped) hdr->dropped = 0ull;
}
// nrs_diffuse_count: the living particles per kind, one workgroup, integer sums
static __global__ __launch_bounds__(SCAN_BLOCK) void k_diffuse_kinds(const uint32_t *__restrict__ kind, DiffuseHeader *__restrict__ hdr)
{
    __shared__ uint32_t wsum[SCAN_BLOCK / 64];
    const uint32_t n = hdr->alive;
    uint32_t c[3] = {0u, 0u, 0u};
    for (uint32_t d = threadIdx.x; d < n; d += SCAN_BLOCK) {
        const uint32_t k = kind[d];
        c[0] += k == 0u; c[1] += k == 1u; c[2] += k == 2u;
    }
    uint32_t tot[3];
    for (int a = 0; a < 3; ++a) block_scan<SCAN_BLOCK>(c[a], wsum, &tot[a]);
    if (threadIdx.x == 0) { hdr->byKind[0] = tot[0]; hdr->byKind[1] = tot[1]; hdr->byKind[2] = tot[2]; }
}

} // namespace nrs
