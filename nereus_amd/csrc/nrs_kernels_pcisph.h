// nrs_kernels_pcisph.h — list-driven kernels of the PCISPH chain (Muller kernels).
//
// The chain is: the step's one density scan (k_density_tiled<..., WIDE>, the launch of the IISPH chain) publishes hit lists that keep
// every candidate with length(r)^2 <= h^2 at the step's start positions; the advection launch takes the non-pressure forces from them
// (forces_from_hits, as k_displacement_lists does); every solver iteration is two launches over the same lists — A, the predicted
// density and the pressure update, and B, the pressure force and the next predicted positions.  Each applies the tests of the
// definition (nrs_kernels_ref.h, "PCISPH": j != i, length(x_i - x_j) < h at the start positions, length(x*_i - x*_j) < h at the
// predicted ones) and forms the sums in the order of the reference-order walks (one partial per (cell, kind) group, fluid before
// boundary inside a cell), so both paths give the same bits.  A particle whose list overflowed takes pci_density_walk / pci_pforce_walk,
// the functions the k_pci_*_ref kernels call.
#pragma once
#include "nrs_kernels_iisph.h"

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
template <typename R, int KSET, bool HAS_B>
NRS_DEV void pci_density_lists_particle(const Params<R> &P, const GridView<R> &G, const PciArrays<R> &A, const HitBuffer &hb,
                                        const typename Vec4T<R>::type *__restrict__ sPos, uint32_t i)
{
    static_assert(KSET == KS_MULLER, "list-driven PCISPH kernels: Muller kernels only (the Monaghan support is 2h, Ctx::Features::listKernels)");
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const V3<R> xs1 = xyz<R>(A.xsIn[i]);
    const R ir = P.interactionRadius, kp = P.kpoly, pm = P.particleMass, rd = P.restDensity;
    const HitCounts hc = unpack_counts(hb.counts[i]);
    R rs;
    if (hc.over) {
        rs = pci_density_walk<R, KSET, HAS_B>(P, G, sPos, A.xsIn, i, pos1, xs1);
    } else {
        rs = (R)0.0;
        rs += pm * W_dens<R, KSET>(mk3<R>(0, 0, 0), ir, kp);
        R part = (R)0.0;
        if (!HAS_B || hc.nb == 0) { // no boundary hits: the fluid entries alone, batched, one partial per cell tag
            uint32_t prevTag = 0xffffffffu;
            struct Nb { typename Vec4T<R>::type q, x; };
            walk_fluid_batched(hb.hits + i, hb.stride, hc.nf, [&](uint32_t j) { return Nb{sPos[j], A.xsIn[j]}; },
                               [&](uint32_t j, uint32_t tag, const Nb &nb) {
                                   if (tag != prevTag) { rs += part; part = (R)0.0; prevTag = tag; }
                                   if (j == i) return;
                                   const V3<R> d0 = pos1 - xyz<R>(nb.q);
                                   if (!(length_listed(dot(d0, d0)) < ir)) return;
                                   const V3<R> d = xs1 - xyz<R>(nb.x);
                                   if (length(d) < ir) part += pm * W_dens<R, KSET>(d, ir, kp);
                               });
        } else { // (cell, kind) groups in the reference's order, every partial into the one total
            for_each_hit(hb.hits + i, hb.stride, hc, [&](uint32_t j, bool isB, bool fresh) {
                if (fresh) { rs += part; part = (R)0.0; }
                if (HAS_B && isB) {
                    const typename Vec4T<R>::type b = G.sB[j];
                    if (!(length(pos1 - xyz<R>(b)) < ir)) return;
                    const V3<R> d = xs1 - xyz<R>(b);
                    if (length(d) < ir) part += (rd * b.w) * W_dens<R, KSET>(d, ir, kp);
                } else if (j != i) {
                    if (!(length(pos1 - xyz<R>(sPos[j])) < ir)) return;
                    const V3<R> d = xs1 - xyz<R>(A.xsIn[j]);
                    if (length(d) < ir) part += pm * W_dens<R, KSET>(d, ir, kp);
                }
            });
        }
        rs += part;
    }
    pci_pressure_update<R>(P, A, i, rs);
}
template <typename R, int KSET, bool HAS_B, bool WALLS = false>
__global__ __launch_bounds__(BLOCK) void k_pci_density_lists(Params<R> P, GridView<R> G, PciArrays<R> A, HitBuffer hb,
                                                             const typename Vec4T<R>::type *__restrict__ sPos, uint32_t n, WallList wl,
                                                             uint32_t wallBlocks)
{
    wall_split<HAS_B, WALLS>(hb, wl, wallBlocks, n, [&](auto hasB, uint32_t i) {
        pci_density_lists_particle<R, KSET, decltype(hasB)::value>(P, G, A, hb, sPos, i);
    });
}

// ---- iteration launch B: pressure force, x* = x + dt (vel_adv + dt Fp / m) into the other buffer ------------------------------------
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
