// nrs_kernels_track.h — the device side of particle tracking (include/nereus_hip.h "particle identity and attributes"; DESIGN.md
// "Particle identity and attributes"): the gather that carries id, birth and the attribute record through a step's sort, the fill of
// new slots, the inverse map of nrs_track_locate and the SPH diffusion of the record.  The rules (which slots are new, which ids they
// get, what is refused) are nrs_host_track.h's; emission and the cull move the tracked arrays inside their own kernels
// (nrs_kernels_inflow.h).  No atomics: ids are unique, so every store of the inverse map has one writer; every sum has one accumulator
// per channel and a fixed order.
#pragma once
#include "nrs_host_track.h"
#include "nrs_kernels_sample.h"

namespace nrs {

// the tracked arrays of one buffer set, in the order of the particle arrays they belong to; rec: null without NRS_TRACK_ATTR
template <typename R> struct TrackView {
    typedef typename Vec4T<R>::type T4;
    uint32_t *id, *birth;
    T4 *rec;
};

// behind a step's reorder: sorted slot s holds the particle that was at index[s]
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_track_gather(const uint32_t *__restrict__ index, TrackView<R> from, TrackView<R> to, uint32_t n)
{
    const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = index[s];
    to.id[s] = from.id[i];
    to.birth[s] = from.birth[i];
    if (to.rec) to.rec[s] = from.rec[i];
}

// slots [first, first + count): id = firstId + (slot - first), one birth, one record
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_track_fill(TrackView<R> to, uint32_t first, uint32_t count, uint32_t firstId, uint32_t birth, typename Vec4T<R>::type val)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= count) return;
    to.id[first + t] = firstId + t;
    to.birth[first + t] = birth;
    if (to.rec) to.rec[first + t] = val;
}

// nrs_track_locate: slotOf (all NRS_TRACK_NONE before) gets the slot of every living id in [firstId, firstId + count)
static __global__ __launch_bounds__(BLOCK) void k_track_locate(const uint32_t *__restrict__ id, uint32_t n, uint64_t firstId, uint32_t count, uint32_t *__restrict__ slotOf)
{
    const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n) return;
    const uint64_t v = id[s];
    if (v < firstId) return;
    const uint64_t k = v - firstId;
    if (k < (uint64_t)count) slotOf[k] = s;
}

// ---- nrs_track_diffuse ----------------------------------------------------------------------------------------------------------------------------
template <typename R> struct TrackDiffuseArgs {
    R kappa[4], dt;
};
// One explicit Euler step of da/dt = kappa_c lap a on the record, the Laplacian of Brookshaw / Cleary and Monaghan with a uniform
// coefficient.  One thread per slot i of the sampler's sorted fluid (sPos, G); sIndex[i]: the particle's place in the current order,
// where its record lives; rho: the density at the sorted particles (k_sample_points at sPos).  Cells z, y, x ascending, j ascending,
// one accumulator per channel; w_ij == w_ji bit for bit and the differences are exact negatives: a pair exchanges equal and opposite
// amounts before the sums round.
template <typename R, int KSET>
__global__ __launch_bounds__(BLOCK) void k_track_diffuse(Params<R> P, GridView<R> G, const typename Vec4T<R>::type *__restrict__ sPos,
                                                         const uint32_t *__restrict__ sIndex, const R *__restrict__ rho,
                                                         const typename Vec4T<R>::type *__restrict__ recIn, typename Vec4T<R>::type *__restrict__ recOut,
                                                         TrackDiffuseArgs<R> A, uint32_t n)
{
    typedef typename Vec4T<R>::type T4;
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t pi = sIndex[i];
    const T4 ai = recIn[pi];
    const V3<R> x = xyz<R>(sPos[i]);
    if (!finite3<R>(x)) { recOut[pi] = ai; return; }
    const R h = P.interactionRadius, m = P.particleMass, rho0 = P.restDensity;
    const R eta2 = (R)0.01 * (h * h);
    const R rhoi = rho[i];
    const bool on0 = A.kappa[0] != (R)0, on1 = A.kappa[1] != (R)0, on2 = A.kappa[2] != (R)0, on3 = A.kappa[3] != (R)0;
    R acc0 = (R)0, acc1 = (R)0, acc2 = (R)0, acc3 = (R)0;
    const I3 gp = calcGridPos<R>(P, x);
    for (int z = -1; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int c = -1; c <= 1; c++) {
                const uint32_t hsh = calcGridHash<R>(P, (int)((uint32_t)gp.x + (uint32_t)c), (int)((uint32_t)gp.y + (uint32_t)y), (int)((uint32_t)gp.z + (uint32_t)z));
                const uint32_t s = G.cellStart[hsh];
                if (s == CELL_EMPTY) continue;
                const uint32_t e = G.cellEnd[hsh];
                if (!run_ok<R>(G, s, e)) continue;
                for (uint32_t j = s; j < e; ++j) {
                    if (j == i) continue;
                    const V3<R> d = x - xyz<R>(sPos[j]);
                    const float len = length(d);
                    if (!(len < h) || len == 0.0f) continue;
                    const V3<R> g = W_grad<R, KSET>(d, h, P.kpoly_grad);
                    const R dg = d.x * g.x + d.y * g.y + d.z * g.z;
                    const R r = (R)len;
                    const R w = (m / (rhoi * rho[j])) * (dg / (r * r + eta2));
                    const T4 aj = recIn[sIndex[j]];
                    if (on0) acc0 += (ai.x - aj.x) * w;
                    if (on1) acc1 += (ai.y - aj.y) * w;
                    if (on2) acc2 += (ai.z - aj.z) * w;
                    if (on3) acc3 += (ai.w - aj.w) * w;
                }
            }
    const R two = (R)2 * A.dt;
    T4 o = ai;
    if (on0) o.x = ai.x + ((two * A.kappa[0]) * rho0) * acc0;
    if (on1) o.y = ai.y + ((two * A.kappa[1]) * rho0) * acc1;
    if (on2) o.z = ai.z + ((two * A.kappa[2]) * rho0) * acc2;
    if (on3) o.w = ai.w + ((two * A.kappa[3]) * rho0) * acc3;
    recOut[pi] = o;
}

} // namespace nrs
