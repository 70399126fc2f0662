// nrs_kernels_dfsph.h — the neighbour passes of the DFSPH chain.
//
// The step's one density scan publishes the wide hit lists (as for PCISPH and PBF); the factor launch and every iteration of both
// solves — A, the divergence (or predicted density) and kappa, and B, the velocity correction in place — walk those lists.  Every
// position is the step's start position, so each hit is tested once, length(x_i - x_j) < h, j != i by sorted slot, and the sums are
// formed in the order of the reference-order walks (one partial per (cell, kind) group, fluid before boundary inside a cell): both
// paths give the same bits.  The walks themselves are the shared ones (nrs_kernels_walk.h); the passes below supply their terms (the
// term functions of nrs_kernels_ref.h, "DFSPH").
#pragma once
#include "nrs_kernels_pbf.h"

namespace nrs {

// what the DFSPH passes share: every term is a function of d = x_i - x_j at the start positions
template <typename R, int KSET> struct DfsphPassBase {
    typedef R Real;
    typedef typename Vec4T<R>::type T4;
    static constexpr int KS = KSET;
    static constexpr bool WALLED = true;
    Params<R> P;
    DfsphArrays<R> A;
};
// ---- the factor launch: alpha_i = 1 / D_i -----------------------------------------------------------------------------------------
template <typename R, int KSET> struct DfsphFactorPass : DfsphPassBase<R, KSET> {
    typedef typename Vec4T<R>::type T4;
    typedef DfsphFac<R> Acc;
    struct Own {};
    struct Nb {};
    NRS_DEV Own own(uint32_t, V3<R>) const { return Own{}; }
    NRS_DEV Acc zero() const { return dfsph_fac_zero<R>(); }
    NRS_DEV Acc start(const Own &) const { return zero(); }
    NRS_DEV Nb gather(uint32_t j) const { return Nb{}; }
    NRS_DEV void fluid(const Own &, V3<R> pos1, const T4 &q, const Nb &nb, float, Acc &part) const { dfsph_fac_fluid<R, KSET>(this->P, pos1 - xyz<R>(q), part); }
    NRS_DEV void boundary(const Own &, V3<R> pos1, uint32_t, const T4 &b, Acc &part) const
    {
        dfsph_fac_boundary<R, KSET>(this->P, pos1 - xyz<R>(b), this->P.restDensity * b.w, part);
    }
    NRS_DEV void store(uint32_t i, V3<R>, const Own &, const Acc &t) const { dfsph_fac_store<R>(this->A, i, t); }
};

// ---- iteration launch A: div_i -> e_i, kappa_i, K_i (DENS: rho_adv).  MOVING: the boundary term with the wall velocities bU, sorted as
// G.sB, (u_i - u_b) . g_ib (dfsph_div_boundary_mv, nrs_kernels_bodies.h includes this header and instantiates it) -----------------------
template <typename R, int KSET> NRS_DEV R dfsph_div_boundary_mv(const Params<R> &P, V3<R> d, R psi, V3<R> ui, V3<R> ub)
{
    return pbf_dot<R>(ui - ub, dfsph_g<R, KSET>(P, d, psi));
}
template <typename R, int KSET, bool DENS, bool MOVING = false> struct DfsphDivPass : DfsphPassBase<R, KSET> {
    typedef typename Vec4T<R>::type T4;
    typename std::conditional<MOVING, const T4 *, WalkUnused>::type bU; // the sorted wall velocities
    int phase;
    typedef R Acc;
    struct Own { V3<R> u1; };
    struct Nb { T4 u; };
    NRS_DEV Own own(uint32_t i, V3<R>) const { return Own{xyz<R>(this->A.u[i])}; }
    NRS_DEV Acc zero() const { return (R)0.0; }
    NRS_DEV Acc start(const Own &) const { return zero(); }
    NRS_DEV Nb gather(uint32_t j) const { return Nb{this->A.u[j]}; }
    NRS_DEV void fluid(const Own &o, V3<R> pos1, const T4 &q, const Nb &nb, float, Acc &part) const
    {
        part += dfsph_div_fluid<R, KSET>(this->P, pos1 - xyz<R>(q), o.u1, xyz<R>(nb.u));
    }
    NRS_DEV void boundary(const Own &o, V3<R> pos1, uint32_t j, const T4 &b, Acc &part) const
    {
        const R psi = this->P.restDensity * b.w;
        if constexpr (MOVING) part += dfsph_div_boundary_mv<R, KSET>(this->P, pos1 - xyz<R>(b), psi, o.u1, xyz<R>(bU[j]));
        else part += dfsph_div_boundary<R, KSET>(this->P, pos1 - xyz<R>(b), psi, o.u1);
    }
    NRS_DEV void store(uint32_t i, V3<R>, const Own &, Acc div) const { dfsph_div_store<R, DENS>(this->P, this->A, i, div, phase); }
};

// ---- iteration launch B: u_i -= dt (sum_j (kappa_i + kappa_j) g_ij + sum_b kappa_i g_ib), in place --------------------------------
// (kept hand-written: in the shared form of nrs_kernels_walk.h the fp32 list kernel with boundary code and without wall workgroups needs
// more than 96 VGPRs and loses a wave, DESIGN.md "One neighbour walk")
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
