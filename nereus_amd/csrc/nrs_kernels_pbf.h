// nrs_kernels_pbf.h — list-driven kernels of the PBF chain (Muller kernels).
//
// The chain is PCISPH's (nrs_kernels_pcisph.h): the step's one density scan publishes the wide hit lists, the advection launch is
// k_pci_advect_lists, and every solver iteration is two launches over the same lists — A, the predicted density and lambda, and B, the
// position correction into the other predicted-position buffer.  The XSPH launch of the integration stage walks the fluid entries only.
// Each applies the tests of the definition (nrs_kernels_ref.h, "PBF": j != i, length(x_i - x_j) < h at the start positions,
// length(x*_i - x*_j) < h at the predicted ones) and forms the sums in the order of the reference-order walks (one partial per
// (cell, kind) group, fluid before boundary inside a cell), so both paths give the same bits.  A particle whose list overflowed takes
// pbf_lambda_walk / pbf_correct_walk / pbf_xsph_walk, the functions the k_pbf_*_ref kernels call.
#pragma once
#include "nrs_kernels_pcisph.h"

namespace nrs {

// ---- iteration launch A: rho*, lambda = -C / (D + eps), e_i --------------------------------------------------------------------------
template <typename R, int KSET, bool HAS_B>
NRS_DEV void pbf_lambda_lists_particle(const Params<R> &P, const GridView<R> &G, const PbfArrays<R> &A, const HitBuffer &hb,
                                       const typename Vec4T<R>::type *__restrict__ sPos, uint32_t i)
{
    static_assert(KSET == KS_MULLER, "list-driven PBF kernels: Muller kernels only (the Monaghan support is 2h, Ctx::Features::listKernels)");
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const V3<R> xs1 = xyz<R>(A.xsIn[i]);
    const R ir = P.interactionRadius, rd = P.restDensity;
    const HitCounts hc = unpack_counts(hb.counts[i]);
    PbfSums<R> t;
    if (hc.over) {
        t = pbf_lambda_walk<R, KSET, HAS_B>(P, G, sPos, A.xsIn, i, pos1, xs1);
    } else {
        t = pbf_zero<R>();
        t.rho += P.particleMass * W_dens<R, KSET>(mk3<R>(0, 0, 0), ir, P.kpoly);
        PbfSums<R> part = pbf_zero<R>();
        if (!HAS_B || hc.nb == 0) { // no boundary hits: the fluid entries alone, batched, one partial per cell tag
            uint32_t prevTag = 0xffffffffu;
            struct Nb { typename Vec4T<R>::type q, x; };
            walk_fluid_batched(hb.hits + i, hb.stride, hc.nf, [&](uint32_t j) { return Nb{sPos[j], A.xsIn[j]}; },
                               [&](uint32_t j, uint32_t tag, const Nb &nb) {
                                   if (tag != prevTag) { t.add(part); part = pbf_zero<R>(); prevTag = tag; }
                                   if (j == i) return;
                                   const V3<R> d0 = pos1 - xyz<R>(nb.q);
                                   if (!(length_listed(dot(d0, d0)) < ir)) return;
                                   pbf_lambda_fluid<R, KSET>(P, xs1 - xyz<R>(nb.x), part);
                               });
        } else { // (cell, kind) groups in the reference's order, every partial into the one total
            for_each_hit(hb.hits + i, hb.stride, hc, [&](uint32_t j, bool isB, bool fresh) {
                if (fresh) { t.add(part); part = pbf_zero<R>(); }
                if (HAS_B && isB) {
                    const typename Vec4T<R>::type b = G.sB[j];
                    if (!(length(pos1 - xyz<R>(b)) < ir)) return;
                    pbf_lambda_boundary<R, KSET>(P, xs1 - xyz<R>(b), rd * b.w, part);
                } else if (j != i) {
                    if (!(length(pos1 - xyz<R>(sPos[j])) < ir)) return;
                    pbf_lambda_fluid<R, KSET>(P, xs1 - xyz<R>(A.xsIn[j]), part);
                }
            });
        }
        t.add(part);
    }
    pbf_lambda_store<R>(P, A, i, t);
}
template <typename R, int KSET, bool HAS_B, bool WALLS = false>
__global__ __launch_bounds__(BLOCK) void k_pbf_lambda_lists(Params<R> P, GridView<R> G, PbfArrays<R> A, HitBuffer hb,
                                                            const typename Vec4T<R>::type *__restrict__ sPos, uint32_t n, WallList wl,
                                                            uint32_t wallBlocks)
{
    wall_split<HAS_B, WALLS>(hb, wl, wallBlocks, n, [&](auto hasB, uint32_t i) {
        pbf_lambda_lists_particle<R, KSET, decltype(hasB)::value>(P, G, A, hb, sPos, i);
    });
}

// ---- iteration launch B: dx_i = sum_j (lambda_i + lambda_j) g_ij + sum_b lambda_i g_ib, x* + dx into the other buffer ------------------
template <typename R, int KSET, bool HAS_B, bool TENS = false>
NRS_DEV void pbf_correct_lists_particle(const Params<R> &P, const GridView<R> &G, const PbfArrays<R> &A, const HitBuffer &hb,
                                        const typename Vec4T<R>::type *__restrict__ sPos, uint32_t i, PbfTensile<R> T = PbfTensile<R>{})
{
    static_assert(KSET == KS_MULLER, "list-driven PBF kernels: Muller kernels only (the Monaghan support is 2h, Ctx::Features::listKernels)");
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const V3<R> xs1 = xyz<R>(A.xsIn[i]);
    const R li = A.lambda[i];
    const R ir = P.interactionRadius, rd = P.restDensity;
    const HitCounts hc = unpack_counts(hb.counts[i]);
    V3<R> dx = mk3<R>(0, 0, 0);
    if (hc.over) {
        dx = pbf_correct_walk<R, KSET, HAS_B, TENS>(P, G, sPos, A.xsIn, A.lambda, i, pos1, xs1, li, T);
    } else {
        V3<R> part = mk3<R>(0, 0, 0);
        if (!HAS_B || hc.nb == 0) {
            uint32_t prevTag = 0xffffffffu;
            struct Nb { typename Vec4T<R>::type q, x; R lj; };
            walk_fluid_batched(hb.hits + i, hb.stride, hc.nf, [&](uint32_t j) { return Nb{sPos[j], A.xsIn[j], A.lambda[j]}; },
                               [&](uint32_t j, uint32_t tag, const Nb &nb) {
                                   if (tag != prevTag) { dx = dx + part; part = mk3<R>(0, 0, 0); prevTag = tag; }
                                   if (j == i) return;
                                   const V3<R> d0 = pos1 - xyz<R>(nb.q);
                                   if (!(length_listed(dot(d0, d0)) < ir)) return;
                                   part = part + pbf_correct_term<R, KSET, TENS>(P, xs1 - xyz<R>(nb.x), li, nb.lj, T);
                               });
        } else {
            for_each_hit(hb.hits + i, hb.stride, hc, [&](uint32_t j, bool isB, bool fresh) {
                if (fresh) { dx = dx + part; part = mk3<R>(0, 0, 0); }
                if (HAS_B && isB) {
                    const typename Vec4T<R>::type b = G.sB[j];
                    if (!(length(pos1 - xyz<R>(b)) < ir)) return;
                    part = part + pbf_correct_boundary<R, KSET>(P, xs1 - xyz<R>(b), rd * b.w, li);
                } else if (j != i) {
                    if (!(length(pos1 - xyz<R>(sPos[j])) < ir)) return;
                    part = part + pbf_correct_term<R, KSET, TENS>(P, xs1 - xyz<R>(A.xsIn[j]), li, A.lambda[j], T);
                }
            });
        }
        dx = dx + part;
    }
    pbf_correct_store<R>(A, i, xs1, dx);
}
template <typename R, int KSET, bool HAS_B, bool WALLS = false>
__global__ __launch_bounds__(BLOCK) void k_pbf_correct_lists(Params<R> P, GridView<R> G, PbfArrays<R> A, HitBuffer hb,
                                                             const typename Vec4T<R>::type *__restrict__ sPos, uint32_t n, WallList wl,
                                                             uint32_t wallBlocks)
{
    wall_split<HAS_B, WALLS>(hb, wl, wallBlocks, n, [&](auto hasB, uint32_t i) {
        pbf_correct_lists_particle<R, KSET, decltype(hasB)::value>(P, G, A, hb, sPos, i);
    });
}

// launch B with the tensile correction s_corr (fluid pairs: lambda_i + lambda_j + s_ij), k_pbf_correct_lists otherwise
template <typename R, int KSET, bool HAS_B, bool WALLS = false>
__global__ __launch_bounds__(BLOCK) void k_pbf_correct_s_lists(Params<R> P, GridView<R> G, PbfArrays<R> A, PbfTensile<R> T, HitBuffer hb,
                                                               const typename Vec4T<R>::type *__restrict__ sPos, uint32_t n, WallList wl,
                                                               uint32_t wallBlocks)
{
    wall_split<HAS_B, WALLS>(hb, wl, wallBlocks, n, [&](auto hasB, uint32_t i) {
        pbf_correct_lists_particle<R, KSET, decltype(hasB)::value, true>(P, G, A, hb, sPos, i, T);
    });
}

// ---- XSPH (integration stage, c > 0): fluid entries only, so one plain launch over every slot (no wall workgroups; the counts of a
// deferred particle are complete, k_density_tiled) ---------------------------------------------------------------------------------------
template <typename R, int KSET>
__global__ __launch_bounds__(BLOCK) void k_pbf_xsph_lists(Params<R> P, GridView<R> G, HitBuffer hb,
                                                          const typename Vec4T<R>::type *__restrict__ sPos,
                                                          const typename Vec4T<R>::type *__restrict__ xs,
                                                          typename Vec4T<R>::type *__restrict__ vel, R c, uint32_t n)
{
    static_assert(KSET == KS_MULLER, "list-driven PBF kernels: Muller kernels only (the Monaghan support is 2h, Ctx::Features::listKernels)");
    const uint32_t i = xcd_tile(blockIdx.x, gridDim.x) * BLOCK + threadIdx.x;
    if (i >= n) return;
    const V3<R> pos1 = xyz<R>(sPos[i]), xs1 = xyz<R>(xs[i]);
    const V3<R> v1 = pbf_vel<R>(P, xs1, pos1);
    const R ir = P.interactionRadius;
    const HitCounts hc = unpack_counts(hb.counts[i]);
    V3<R> sum = mk3<R>(0, 0, 0);
    if (hc.over) {
        sum = pbf_xsph_walk<R, KSET>(P, G, sPos, xs, i, pos1, xs1, v1);
    } else {
        V3<R> part = mk3<R>(0, 0, 0);
        uint32_t prevTag = 0xffffffffu;
        struct Nb { typename Vec4T<R>::type q, x; };
        walk_fluid_batched(hb.hits + i, hb.stride, hc.nf, [&](uint32_t j) { return Nb{sPos[j], xs[j]}; },
                           [&](uint32_t j, uint32_t tag, const Nb &nb) {
                               if (tag != prevTag) { sum = sum + part; part = mk3<R>(0, 0, 0); prevTag = tag; }
                               if (j == i) return;
                               const V3<R> xj = xyz<R>(nb.q);
                               const V3<R> d0 = pos1 - xj;
                               if (!(length_listed(dot(d0, d0)) < ir)) return;
                               const V3<R> xsj = xyz<R>(nb.x);
                               part = part + pbf_xsph_fluid<R, KSET>(P, xs1 - xsj, pbf_vel<R>(P, xsj, xj), v1);
                           });
        sum = sum + part;
    }
    vel[i] = mk4<R>(v1 + pci_scale<R>(c, sum), (R)0.0);
}

// ---- vorticity confinement (integration stage, eps_v > 0): the two fluid-only launches of nrs_kernels_ref.h "vorticity confinement",
// plain launches over every slot like k_pbf_xsph_lists ----------------------------------------------------------------------------------
template <typename R, int KSET>
__global__ __launch_bounds__(BLOCK) void k_pbf_vorticity_lists(Params<R> P, GridView<R> G, HitBuffer hb,
                                                               const typename Vec4T<R>::type *__restrict__ sPos,
                                                               const typename Vec4T<R>::type *__restrict__ xs,
                                                               typename Vec4T<R>::type *__restrict__ omega, uint32_t n)
{
    static_assert(KSET == KS_MULLER, "list-driven PBF kernels: Muller kernels only (the Monaghan support is 2h, Ctx::Features::listKernels)");
    const uint32_t i = xcd_tile(blockIdx.x, gridDim.x) * BLOCK + threadIdx.x;
    if (i >= n) return;
    const V3<R> pos1 = xyz<R>(sPos[i]), xs1 = xyz<R>(xs[i]);
    const V3<R> u1 = pbf_vel<R>(P, xs1, pos1);
    const R ir = P.interactionRadius;
    const HitCounts hc = unpack_counts(hb.counts[i]);
    V3<R> sum = mk3<R>(0, 0, 0);
    if (hc.over) {
        sum = pbf_vort_walk<R, KSET>(P, G, sPos, xs, i, pos1, xs1, u1);
    } else {
        V3<R> part = mk3<R>(0, 0, 0);
        uint32_t prevTag = 0xffffffffu;
        struct Nb { typename Vec4T<R>::type q, x; };
        walk_fluid_batched(hb.hits + i, hb.stride, hc.nf, [&](uint32_t j) { return Nb{sPos[j], xs[j]}; },
                           [&](uint32_t j, uint32_t tag, const Nb &nb) {
                               if (tag != prevTag) { sum = sum + part; part = mk3<R>(0, 0, 0); prevTag = tag; }
                               if (j == i) return;
                               const V3<R> xj = xyz<R>(nb.q);
                               const V3<R> d0 = pos1 - xj;
                               if (!(length_listed(dot(d0, d0)) < ir)) return;
                               const V3<R> xsj = xyz<R>(nb.x);
                               part = part + pbf_vort_fluid<R, KSET>(P, xs1 - xsj, pbf_vel<R>(P, xsj, xj), u1);
                           });
        sum = sum + part;
    }
    omega[i] = pbf_vort_pack<R>(sum);
}
template <typename R, int KSET>
__global__ __launch_bounds__(BLOCK) void k_pbf_confine_lists(Params<R> P, GridView<R> G, HitBuffer hb,
                                                             const typename Vec4T<R>::type *__restrict__ sPos,
                                                             const typename Vec4T<R>::type *__restrict__ xs,
                                                             const typename Vec4T<R>::type *__restrict__ omega,
                                                             typename Vec4T<R>::type *__restrict__ vel, int velGiven, R epsV, uint32_t n)
{
    static_assert(KSET == KS_MULLER, "list-driven PBF kernels: Muller kernels only (the Monaghan support is 2h, Ctx::Features::listKernels)");
    const uint32_t i = xcd_tile(blockIdx.x, gridDim.x) * BLOCK + threadIdx.x;
    if (i >= n) return;
    const V3<R> pos1 = xyz<R>(sPos[i]), xs1 = xyz<R>(xs[i]);
    const typename Vec4T<R>::type om = omega[i];
    const R wi = om.w;
    const R ir = P.interactionRadius;
    const HitCounts hc = unpack_counts(hb.counts[i]);
    V3<R> sum = mk3<R>(0, 0, 0);
    if (hc.over) {
        sum = pbf_eta_walk<R, KSET>(P, G, sPos, xs, omega, i, pos1, xs1, wi);
    } else {
        V3<R> part = mk3<R>(0, 0, 0);
        uint32_t prevTag = 0xffffffffu;
        struct Nb { typename Vec4T<R>::type q, x; R wj; };
        walk_fluid_batched(hb.hits + i, hb.stride, hc.nf, [&](uint32_t j) { return Nb{sPos[j], xs[j], omega[j].w}; },
                           [&](uint32_t j, uint32_t tag, const Nb &nb) {
                               if (tag != prevTag) { sum = sum + part; part = mk3<R>(0, 0, 0); prevTag = tag; }
                               if (j == i) return;
                               const V3<R> d0 = pos1 - xyz<R>(nb.q);
                               if (!(length_listed(dot(d0, d0)) < ir)) return;
                               part = part + pbf_eta_fluid<R, KSET>(P, xs1 - xyz<R>(nb.x), nb.wj, wi);
                           });
        sum = sum + part;
    }
    const V3<R> v = velGiven ? xyz<R>(vel[i]) : pbf_vel<R>(P, xs1, pos1);
    vel[i] = mk4<R>(pbf_confine<R>(P, v, sum, om, epsV), (R)0.0);
}

} // namespace nrs
