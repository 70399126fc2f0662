// nrs_kernels_walk.h — the two neighbour walks of the PCISPH, PBF, DFSPH and Akinci-normals passes, each written once.
//
// A pass (nrs_kernels_pcisph.h, _pbf.h, _dfsph.h, _akinci.h) is a small struct that is the kernel's argument and supplies
// only what differs between the passes:
//   Real, KS, WALLED   the precision, the kernel set, and whether the pass has a boundary term (false: fluid neighbours only — the walks
//                      are instantiated with HAS_B = false and the list kernel is launched plain, without wall workgroups);
//   Acc, zero()        the accumulator (R, V3<R>, PbfSums<R>, DfsphFac<R>; added with walk_add) and its zero;
//   start(own)         the total before the first cell: zero(), or the self term (the W(0) of the density sums);
//   Own, own(i, pos1)  what particle i reads of itself (x*_i, p_i, u_i, ...);
//   Nb, gather(j)      what is read of a fluid neighbour besides its sorted position q = sPos[j], which the walk reads: xsIn[j], pres[j], ...;
//   fluid(own, pos1, q, nb, rlen, part)    the term of a fluid neighbour that passed the start-position test (rlen: its length there);
//   boundary(own, pos1, j, b, part)        ... of the boundary particle b = G.sB[j] that passed it;
//   store(i, pos1, own, total)             what the launch writes.
// The walks apply the start-position test, j != i (by sorted slot) and length(x_i - x_j) < h, and fix the order of summation: the 27
// cells z, y, x ascending, in each a fluid partial (j ascending) and then a boundary partial, each added to the running total.  A test
// at predicted positions (PCISPH, PBF) is part of the pass's term.
//   walk_cells   the cells themselves, the reference's order: the k_walk_ref kernels and the particles whose hit list overflowed;
//   walk_hits    the hit lists of the step's density scan (Muller kernels): the same partials, so both give the same bits.
#pragma once
#include "nrs_kernels_iisph.h"

namespace nrs {

struct WalkUnused {}; // the type of a pass member that one of its template variants does not have

NRS_DEV void walk_add(float &t, float c) { t += c; }
NRS_DEV void walk_add(double &t, double c) { t += c; }
template <typename R> NRS_DEV void walk_add(V3<R> &t, const V3<R> &c) { t = t + c; }
template <typename S> NRS_DEV auto walk_add(S &t, const S &c) -> decltype(t.add(c)) { t.add(c); }

template <bool HAS_B, typename Pass>
NRS_DEV typename Pass::Acc walk_cells(const Pass &pass, const GridView<typename Pass::Real> &G,
                                      const typename Vec4T<typename Pass::Real>::type *__restrict__ sPos, uint32_t i,
                                      V3<typename Pass::Real> pos1, const typename Pass::Own &own)
{
    typedef typename Pass::Real R;
    const R ir = pass.P.interactionRadius;
    const I3 gp = calcGridPos<R>(pass.P, pos1);
    typename Pass::Acc t = pass.start(own);
    for (int z = -1; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int x = -1; x <= 1; x++) {
                const uint32_t h = calcGridHash<R>(pass.P, gp.x + x, gp.y + y, gp.z + z);
                typename Pass::Acc c = pass.zero();
                const uint32_t s = G.cellStart[h];
                if (s != CELL_EMPTY) {
                    const uint32_t e = G.cellEnd[h];
                    for (uint32_t j = s; j < e; ++j) {
                        if (j == i) continue;
                        const typename Vec4T<R>::type q = sPos[j];
                        const float rlen = length(pos1 - xyz<R>(q));
                        if (!(rlen < ir)) continue;
                        pass.fluid(own, pos1, q, pass.gather(j), rlen, c);
                    }
                }
                walk_add(t, c);
                if constexpr (HAS_B) {
                    typename Pass::Acc cb = pass.zero();
                    const uint32_t sb = G.bCellStart[h];
                    if (sb != CELL_EMPTY) {
                        const uint32_t e = G.bCellEnd[h];
                        for (uint32_t j = sb; j < e; ++j) {
                            const typename Vec4T<R>::type b = G.sB[j];
                            if (!(length(pos1 - xyz<R>(b)) < ir)) continue;
                            pass.boundary(own, pos1, j, b, cb);
                        }
                    }
                    walk_add(t, cb);
                }
            }
    return t;
}

// Particle i of a list kernel.  An overflowed list: walk_cells.  No boundary hits: the fluid entries alone, batched (every Nb of a batch
// gathered before the first is used), one partial per cell tag, the distance as length_listed.  Otherwise the (cell, kind) groups in the
// reference's order, one partial per group, the distance as length().  The two forms of the distance give the same bits (nrs_math.h).
template <bool HAS_B, typename Pass>
NRS_DEV void walk_hits(const Pass &pass, const GridView<typename Pass::Real> &G, const HitBuffer &hb,
                       const typename Vec4T<typename Pass::Real>::type *__restrict__ sPos, uint32_t i)
{
    typedef typename Pass::Real R;
    struct Hit { typename Vec4T<R>::type q; typename Pass::Nb nb; };
    static_assert(Pass::KS == KS_MULLER, "list-driven kernels: Muller kernels only (the Monaghan support is 2h, Ctx::Features::listKernels)");
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const typename Pass::Own own = pass.own(i, pos1);
    const R ir = pass.P.interactionRadius;
    const HitCounts hc = unpack_counts(hb.counts[i]);
    typename Pass::Acc t;
    if (hc.over) {
        t = walk_cells<HAS_B>(pass, G, sPos, i, pos1, own);
    } else {
        t = pass.start(own);
        typename Pass::Acc part = pass.zero();
        if (!HAS_B || hc.nb == 0) {
            uint32_t prevTag = 0xffffffffu;
            walk_fluid_batched(hb.hits + i, hb.stride, hc.nf, [&](uint32_t j) { return Hit{sPos[j], pass.gather(j)}; },
                               [&](uint32_t j, uint32_t tag, const Hit &hit) {
                                   if (tag != prevTag) { walk_add(t, part); part = pass.zero(); prevTag = tag; }
                                   if (j == i) return;
                                   const V3<R> d0 = pos1 - xyz<R>(hit.q);
                                   const float rlen = length_listed(dot(d0, d0));
                                   if (!(rlen < ir)) return;
                                   pass.fluid(own, pos1, hit.q, hit.nb, rlen, part);
                               });
        } else {
            for_each_hit(hb.hits + i, hb.stride, hc, [&](uint32_t j, bool isB, bool fresh) {
                if (fresh) { walk_add(t, part); part = pass.zero(); }
                if (HAS_B && isB) {
                    const typename Vec4T<R>::type b = G.sB[j];
                    if (!(length(pos1 - xyz<R>(b)) < ir)) return;
                    pass.boundary(own, pos1, j, b, part);
                } else if (j != i) {
                    const typename Vec4T<R>::type q = sPos[j];
                    const float rlen = length(pos1 - xyz<R>(q));
                    if (!(rlen < ir)) return;
                    pass.fluid(own, pos1, q, pass.gather(j), rlen, part);
                }
            });
        }
        walk_add(t, part);
    }
    pass.store(i, pos1, own, t);
}

// the reference-order launch of a pass: one sorted slot per thread
template <typename Pass, bool HAS_B>
__global__ __launch_bounds__(BLOCK) void k_walk_ref(Pass pass, GridView<typename Pass::Real> G,
                                                    const typename Vec4T<typename Pass::Real>::type *__restrict__ sPos, uint32_t n)
{
    typedef typename Pass::Real R;
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const typename Pass::Own own = pass.own(i, pos1);
    pass.store(i, pos1, own, walk_cells<HAS_B>(pass, G, sPos, i, pos1, own));
}
// the list-driven launch (wall_split, nrs_kernels_iisph.h); a fluid-only pass: HAS_B = WALLS = false, one plain launch over every slot
// (the wall workgroups exist to keep the boundary code out of the interior waves, and the counts of a deferred particle are complete)
template <typename Pass, bool HAS_B, bool WALLS = false>
__global__ __launch_bounds__(BLOCK) void k_walk_lists(Pass pass, GridView<typename Pass::Real> G, HitBuffer hb,
                                                      const typename Vec4T<typename Pass::Real>::type *__restrict__ sPos, uint32_t n,
                                                      WallList wl, uint32_t wallBlocks)
{
    wall_split<HAS_B, WALLS>(hb, wl, wallBlocks, n, [&](auto hasB, uint32_t i) { walk_hits<decltype(hasB)::value>(pass, G, hb, sPos, i); });
}

} // namespace nrs
