// nrs_kernels_dfsph.h — list-driven kernels of the DFSPH chain (Muller kernels).
//
// The step's one density scan publishes the wide hit lists (as for PCISPH and PBF); the factor launch and every iteration of both
// solves — A, the divergence (or predicted density) and kappa, and B, the velocity correction in place — walk those lists.  Every
// position is the step's start position, so each hit is tested once, length(x_i - x_j) < h, j != i by sorted slot, and the sums are
// formed in the order of the reference-order walks (one partial per (cell, kind) group, fluid before boundary inside a cell): both
// paths give the same bits.  A particle whose list overflowed takes dfsph_factor_walk / dfsph_div_walk / dfsph_vup_walk, the
// functions the k_dfsph_*_ref kernels call (nrs_kernels_ref.h, "DFSPH").
#pragma once
#include "nrs_kernels_pbf.h"

namespace nrs {

// ---- the factor launch: alpha_i = 1 / D_i -----------------------------------------------------------------------------------------
template <typename R, int KSET, bool HAS_B>
NRS_DEV void dfsph_factor_lists_particle(const Params<R> &P, const GridView<R> &G, const DfsphArrays<R> &A, const HitBuffer &hb,
                                         const typename Vec4T<R>::type *__restrict__ sPos, uint32_t i)
{
    static_assert(KSET == KS_MULLER, "list-driven DFSPH kernels: Muller kernels only (the Monaghan support is 2h, Ctx::Features::listKernels)");
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const R ir = P.interactionRadius, rd = P.restDensity;
    const HitCounts hc = unpack_counts(hb.counts[i]);
    DfsphFac<R> t;
    if (hc.over) {
        t = dfsph_factor_walk<R, KSET, HAS_B>(P, G, sPos, i, pos1);
    } else {
        t = dfsph_fac_zero<R>();
        DfsphFac<R> part = dfsph_fac_zero<R>();
        if (!HAS_B || hc.nb == 0) { // no boundary hits: the fluid entries alone, batched, one partial per cell tag
            uint32_t prevTag = 0xffffffffu;
            struct Nb { typename Vec4T<R>::type q; };
            walk_fluid_batched(hb.hits + i, hb.stride, hc.nf, [&](uint32_t j) { return Nb{sPos[j]}; },
                               [&](uint32_t j, uint32_t tag, const Nb &nb) {
                                   if (tag != prevTag) { t.add(part); part = dfsph_fac_zero<R>(); prevTag = tag; }
                                   if (j == i) return;
                                   const V3<R> d = pos1 - xyz<R>(nb.q);
                                   if (!(length_listed(dot(d, d)) < ir)) return;
                                   dfsph_fac_fluid<R, KSET>(P, d, part);
                               });
        } else { // (cell, kind) groups in the reference's order, every partial into the one total
            for_each_hit(hb.hits + i, hb.stride, hc, [&](uint32_t j, bool isB, bool fresh) {
                if (fresh) { t.add(part); part = dfsph_fac_zero<R>(); }
                if (HAS_B && isB) {
                    const typename Vec4T<R>::type b = G.sB[j];
                    const V3<R> d = pos1 - xyz<R>(b);
                    if (!(length(d) < ir)) return;
                    dfsph_fac_boundary<R, KSET>(P, d, rd * b.w, part);
                } else if (j != i) {
                    const V3<R> d = pos1 - xyz<R>(sPos[j]);
                    if (!(length(d) < ir)) return;
                    dfsph_fac_fluid<R, KSET>(P, d, part);
                }
            });
        }
        t.add(part);
    }
    dfsph_fac_store<R>(A, i, t);
}
template <typename R, int KSET, bool HAS_B, bool WALLS = false>
__global__ __launch_bounds__(BLOCK) void k_dfsph_factor_lists(Params<R> P, GridView<R> G, DfsphArrays<R> A, HitBuffer hb,
                                                              const typename Vec4T<R>::type *__restrict__ sPos, uint32_t n, WallList wl,
                                                              uint32_t wallBlocks)
{
    wall_split<HAS_B, WALLS>(hb, wl, wallBlocks, n, [&](auto hasB, uint32_t i) {
        dfsph_factor_lists_particle<R, KSET, decltype(hasB)::value>(P, G, A, hb, sPos, i);
    });
}

// ---- iteration launch A: div_i -> e_i, kappa_i, K_i (DENS: rho_adv) ---------------------------------------------------------------
template <typename R, int KSET, bool HAS_B, bool DENS>
NRS_DEV void dfsph_div_lists_particle(const Params<R> &P, const GridView<R> &G, const DfsphArrays<R> &A, const HitBuffer &hb,
                                      const typename Vec4T<R>::type *__restrict__ sPos, int phase, uint32_t i)
{
    static_assert(KSET == KS_MULLER, "list-driven DFSPH kernels: Muller kernels only (the Monaghan support is 2h, Ctx::Features::listKernels)");
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const V3<R> u1 = xyz<R>(A.u[i]);
    const R ir = P.interactionRadius, rd = P.restDensity;
    const HitCounts hc = unpack_counts(hb.counts[i]);
    R div;
    if (hc.over) {
        div = dfsph_div_walk<R, KSET, HAS_B>(P, G, sPos, A.u, i, pos1, u1);
    } else {
        div = (R)0.0;
        R part = (R)0.0;
        if (!HAS_B || hc.nb == 0) {
            uint32_t prevTag = 0xffffffffu;
            struct Nb { typename Vec4T<R>::type q, u; };
            walk_fluid_batched(hb.hits + i, hb.stride, hc.nf, [&](uint32_t j) { return Nb{sPos[j], A.u[j]}; },
                               [&](uint32_t j, uint32_t tag, const Nb &nb) {
                                   if (tag != prevTag) { div += part; part = (R)0.0; prevTag = tag; }
                                   if (j == i) return;
                                   const V3<R> d = pos1 - xyz<R>(nb.q);
                                   if (!(length_listed(dot(d, d)) < ir)) return;
                                   part += dfsph_div_fluid<R, KSET>(P, d, u1, xyz<R>(nb.u));
                               });
        } else {
            for_each_hit(hb.hits + i, hb.stride, hc, [&](uint32_t j, bool isB, bool fresh) {
                if (fresh) { div += part; part = (R)0.0; }
                if (HAS_B && isB) {
                    const typename Vec4T<R>::type b = G.sB[j];
                    const V3<R> d = pos1 - xyz<R>(b);
                    if (!(length(d) < ir)) return;
                    part += dfsph_div_boundary<R, KSET>(P, d, rd * b.w, u1);
                } else if (j != i) {
                    const V3<R> d = pos1 - xyz<R>(sPos[j]);
                    if (!(length(d) < ir)) return;
                    part += dfsph_div_fluid<R, KSET>(P, d, u1, xyz<R>(A.u[j]));
                }
            });
        }
        div += part;
    }
    dfsph_div_store<R, DENS>(P, A, i, div, phase);
}
template <typename R, int KSET, bool HAS_B, bool DENS, bool WALLS = false>
__global__ __launch_bounds__(BLOCK) void k_dfsph_div_lists(Params<R> P, GridView<R> G, DfsphArrays<R> A, HitBuffer hb,
                                                           const typename Vec4T<R>::type *__restrict__ sPos, int phase, uint32_t n,
                                                           WallList wl, uint32_t wallBlocks)
{
    wall_split<HAS_B, WALLS>(hb, wl, wallBlocks, n, [&](auto hasB, uint32_t i) {
        dfsph_div_lists_particle<R, KSET, decltype(hasB)::value, DENS>(P, G, A, hb, sPos, phase, i);
    });
}

// ---- iteration launch B: u_i -= dt (sum_j (kappa_i + kappa_j) g_ij + sum_b kappa_i g_ib), in place --------------------------------
template <typename R, int KSET, bool HAS_B>
NRS_DEV void dfsph_vupdate_lists_particle(const Params<R> &P, const GridView<R> &G, const DfsphArrays<R> &A, const HitBuffer &hb,
                                          const typename Vec4T<R>::type *__restrict__ sPos, uint32_t i)
{
    static_assert(KSET == KS_MULLER, "list-driven DFSPH kernels: Muller kernels only (the Monaghan support is 2h, Ctx::Features::listKernels)");
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const typename Vec4T<R>::type u = A.u[i];
    const R ki = A.kappa[i];
    const R ir = P.interactionRadius, rd = P.restDensity;
    const HitCounts hc = unpack_counts(hb.counts[i]);
    V3<R> sum = mk3<R>(0, 0, 0);
    if (hc.over) {
        sum = dfsph_vup_walk<R, KSET, HAS_B>(P, G, sPos, A.kappa, i, pos1, ki);
    } else {
        V3<R> part = mk3<R>(0, 0, 0);
        if (!HAS_B || hc.nb == 0) {
            uint32_t prevTag = 0xffffffffu;
            struct Nb { typename Vec4T<R>::type q; R kj; };
            walk_fluid_batched(hb.hits + i, hb.stride, hc.nf, [&](uint32_t j) { return Nb{sPos[j], A.kappa[j]}; },
                               [&](uint32_t j, uint32_t tag, const Nb &nb) {
                                   if (tag != prevTag) { sum = sum + part; part = mk3<R>(0, 0, 0); prevTag = tag; }
                                   if (j == i) return;
                                   const V3<R> d = pos1 - xyz<R>(nb.q);
                                   if (!(length_listed(dot(d, d)) < ir)) return;
                                   part = part + dfsph_vup_fluid<R, KSET>(P, d, ki, nb.kj);
                               });
        } else {
            for_each_hit(hb.hits + i, hb.stride, hc, [&](uint32_t j, bool isB, bool fresh) {
                if (fresh) { sum = sum + part; part = mk3<R>(0, 0, 0); }
                if (HAS_B && isB) {
                    const typename Vec4T<R>::type b = G.sB[j];
                    const V3<R> d = pos1 - xyz<R>(b);
                    if (!(length(d) < ir)) return;
                    part = part + dfsph_vup_boundary<R, KSET>(P, d, rd * b.w, ki);
                } else if (j != i) {
                    const V3<R> d = pos1 - xyz<R>(sPos[j]);
                    if (!(length(d) < ir)) return;
                    part = part + dfsph_vup_fluid<R, KSET>(P, d, ki, A.kappa[j]);
                }
            });
        }
        sum = sum + part;
    }
    dfsph_vup_store<R>(P, A, i, u, sum);
}
template <typename R, int KSET, bool HAS_B, bool WALLS = false>
__global__ __launch_bounds__(BLOCK) void k_dfsph_vupdate_lists(Params<R> P, GridView<R> G, DfsphArrays<R> A, HitBuffer hb,
                                                               const typename Vec4T<R>::type *__restrict__ sPos, uint32_t n, WallList wl,
                                                               uint32_t wallBlocks)
{
    wall_split<HAS_B, WALLS>(hb, wl, wallBlocks, n, [&](auto hasB, uint32_t i) {
        dfsph_vupdate_lists_particle<R, KSET, decltype(hasB)::value>(P, G, A, hb, sPos, i);
    });
}

} // namespace nrs
