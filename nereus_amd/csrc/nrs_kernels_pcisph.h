// nrs_kernels_pcisph.h — the list-driven advection launch (Muller kernels) and the two neighbour passes of the PCISPH chain.
//
// The chain is: the step's one density scan (k_density_tiled<..., WIDE>, the launch of the IISPH chain) publishes hit lists that keep
// every candidate with length(r)^2 <= h^2 at the step's start positions; the advection launch takes the non-pressure forces from them
// (forces_from_hits, as k_displacement_lists does); every solver iteration is two launches over the same lists — A, the predicted
// density and the pressure update, and B, the pressure force and the next predicted positions.  Each applies the tests of the
// definition (nrs_kernels_ref.h, "PCISPH": j != i, length(x_i - x_j) < h at the start positions, length(x*_i - x*_j) < h at the
// predicted ones) and forms the sums in the order of the reference-order walks (one partial per (cell, kind) group, fluid before
// boundary inside a cell), so both paths give the same bits.  A and B are passes of the shared walks (nrs_kernels_walk.h: walk_hits over
// the lists, walk_cells for the reference-order kernels and for a particle whose list overflowed); only their terms are written here.
#pragma once
#include "nrs_kernels_walk.h"

namespace nrs {

// ---- advection: forces_from_hits + vel_adv, x*0, p = 0, Fp = 0 ---------------------------------------------------------------------
template <typename R, int KSET, bool SURF, bool HAS_B>
NRS_DEV void pci_advect_lists_particle(const Params<R> &P, const GridView<R> &G, const PciArrays<R> &A, const HitBuffer &hb,
                                       const typename Vec4T<R>::type *__restrict__ sPos, const typename Vec4T<R>::type *__restrict__ sVel,
                                       const R *__restrict__ sDens, const R *__restrict__ sPres, uint32_t i)
{
    static_assert(KSET == KS_MULLER, "list-driven PCISPH kernels: Muller kernels only (the Monaghan support is 2h, Ctx::Features::listKernels)");
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const V3<R> vel1 = xyz<R>(sVel[i]);
    const R pres = (R)0.0;
    const R dens = sDens[i];
    const HitCounts hc = unpack_counts(hb.counts[i]);
    ForceAcc<R> F;
    if (hc.over) F = gather_forces<R, KSET, SURF, HAS_B>(P, G, i, pos1, vel1, dens, pres, sPos, sVel, sDens, sPres);
    else F = forces_from_hits<R, KSET, SURF, HAS_B, true>(P, G, sPos, sVel, sDens, sPres, pos1, vel1, dens, pres, hb.hits + i, hb.stride, hc, i);
    pci_advect_store<R>(P, A, i, pos1, vel1, pci_advect_force<R>(P, F));
}
template <typename R, int KSET, bool SURF, bool HAS_B, bool WALLS = false>
__global__ __launch_bounds__(BLOCK) void k_pci_advect_lists(Params<R> P, GridView<R> G, PciArrays<R> A, HitBuffer hb,
                                                            const typename Vec4T<R>::type *__restrict__ sPos,
                                                            const typename Vec4T<R>::type *__restrict__ sVel,
                                                            const R *__restrict__ sDens, const R *__restrict__ sPres, uint32_t n,
                                                            WallList wl, uint32_t wallBlocks)
{
    wall_split<HAS_B, WALLS>(hb, wl, wallBlocks, n, [&](auto hasB, uint32_t i) {
        pci_advect_lists_particle<R, KSET, SURF, decltype(hasB)::value>(P, G, A, hb, sPos, sVel, sDens, sPres, i);
    });
}

// ---- iteration launch A: predicted density, p += delta (rho* - rho0) clamped at 0, e_i ----------------------------------------------
template <typename R, int KSET> struct PciDensityPass {
    typedef R Real;
    typedef typename Vec4T<R>::type T4;
    static constexpr int KS = KSET;
    static constexpr bool WALLED = true;
    Params<R> P;
    PciArrays<R> A;
    typedef R Acc;
    struct Own { V3<R> xs1; };
    struct Nb { T4 x; };
    NRS_DEV Own own(uint32_t i, V3<R>) const { return Own{xyz<R>(A.xsIn[i])}; }
    NRS_DEV Acc zero() const { return (R)0.0; }
    NRS_DEV Acc start(const Own &) const
    {
        R rs = (R)0.0;
        rs += P.particleMass * W_dens<R, KSET>(mk3<R>(0, 0, 0), P.interactionRadius, P.kpoly);
        return rs;
    }
    NRS_DEV Nb gather(uint32_t j) const { return Nb{A.xsIn[j]}; }
    NRS_DEV void fluid(const Own &o, V3<R>, const T4 &, const Nb &nb, float, Acc &part) const
    {
        const R ir = P.interactionRadius;
        const V3<R> d = o.xs1 - xyz<R>(nb.x);
        if (length(d) < ir) part += P.particleMass * W_dens<R, KSET>(d, ir, P.kpoly);
    }
    NRS_DEV void boundary(const Own &o, V3<R>, uint32_t, const T4 &b, Acc &part) const
    {
        const R ir = P.interactionRadius;
        const V3<R> d = o.xs1 - xyz<R>(b);
        if (length(d) < ir) part += (P.restDensity * b.w) * W_dens<R, KSET>(d, ir, P.kpoly);
    }
    NRS_DEV void store(uint32_t i, V3<R>, const Own &, Acc rs) const { pci_pressure_update<R>(P, A, i, rs); }
};

// ---- iteration launch B: pressure force, x* = x + dt (vel_adv + dt Fp / m) into the other buffer ------------------------------------
// (kept hand-written: in the shared form of nrs_kernels_walk.h the fp32 list kernel with boundary code and without wall workgroups needs
// more than 96 VGPRs and loses a wave, DESIGN.md "One neighbour walk")
template <typename R, int KSET, bool HAS_B>
NRS_DEV void pci_pforce_lists_particle(const Params<R> &P, const GridView<R> &G, const PciArrays<R> &A, const HitBuffer &hb,
                                       const typename Vec4T<R>::type *__restrict__ sPos, uint32_t i)
{
    static_assert(KSET == KS_MULLER, "list-driven PCISPH kernels: Muller kernels only (the Monaghan support is 2h, Ctx::Features::listKernels)");
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const V3<R> xs1 = xyz<R>(A.xsIn[i]);
    const R p = A.pres[i];
    const R ir = P.interactionRadius, kpg = P.kpoly_grad, rd = P.restDensity;
    const HitCounts hc = unpack_counts(hb.counts[i]);
    V3<R> fp = mk3<R>(0, 0, 0);
    if (hc.over) {
        fp = pci_pforce_walk<R, KSET, HAS_B>(P, G, sPos, A.xsIn, A.pres, i, pos1, xs1, p);
    } else {
        V3<R> part = mk3<R>(0, 0, 0);
        if (!HAS_B || hc.nb == 0) {
            uint32_t prevTag = 0xffffffffu;
            struct Nb { typename Vec4T<R>::type q, x; R pj; };
            walk_fluid_batched(hb.hits + i, hb.stride, hc.nf, [&](uint32_t j) { return Nb{sPos[j], A.xsIn[j], A.pres[j]}; },
                               [&](uint32_t j, uint32_t tag, const Nb &nb) {
                                   if (tag != prevTag) { fp = fp + part; part = mk3<R>(0, 0, 0); prevTag = tag; }
                                   if (j == i) return;
                                   const V3<R> d0 = pos1 - xyz<R>(nb.q);
                                   if (!(length_listed(dot(d0, d0)) < ir)) return;
                                   const V3<R> d = xs1 - xyz<R>(nb.x);
                                   if (length(d) < ir) part = part + pci_scale<R>(pci_fluid_coef<R>(P, p, nb.pj), W_grad<R, KSET>(d, ir, kpg));
                               });
        } else {
            for_each_hit(hb.hits + i, hb.stride, hc, [&](uint32_t j, bool isB, bool fresh) {
                if (fresh) { fp = fp + part; part = mk3<R>(0, 0, 0); }
                if (HAS_B && isB) {
                    const typename Vec4T<R>::type b = G.sB[j];
                    if (!(length(pos1 - xyz<R>(b)) < ir)) return;
                    const V3<R> d = xs1 - xyz<R>(b);
                    if (length(d) < ir) part = part + pci_scale<R>(pci_boundary_coef<R>(P, rd * b.w, p), W_grad<R, KSET>(d, ir, kpg));
                } else if (j != i) {
                    if (!(length(pos1 - xyz<R>(sPos[j])) < ir)) return;
                    const V3<R> d = xs1 - xyz<R>(A.xsIn[j]);
                    if (length(d) < ir) part = part + pci_scale<R>(pci_fluid_coef<R>(P, p, A.pres[j]), W_grad<R, KSET>(d, ir, kpg));
                }
            });
        }
        fp = fp + part;
    }
    A.forcesP[i] = mk4<R>(fp, (R)0.0);
    A.xsOut[i] = mk4<R>(pci_predict<R>(P, pos1, xyz<R>(A.velAdv[i]), fp), (R)1.0);
}
template <typename R, int KSET, bool HAS_B, bool WALLS = false>
__global__ __launch_bounds__(BLOCK) void k_pci_pforce_lists(Params<R> P, GridView<R> G, PciArrays<R> A, HitBuffer hb,
                                                            const typename Vec4T<R>::type *__restrict__ sPos, uint32_t n, WallList wl,
                                                            uint32_t wallBlocks)
{
    wall_split<HAS_B, WALLS>(hb, wl, wallBlocks, n, [&](auto hasB, uint32_t i) {
        pci_pforce_lists_particle<R, KSET, decltype(hasB)::value>(P, G, A, hb, sPos, i);
    });
}

} // namespace nrs
