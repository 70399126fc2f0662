// nrs_kernels_pbf.h — the neighbour passes of the PBF chain.
//
// The chain is PCISPH's (nrs_kernels_pcisph.h): the step's one density scan publishes the wide hit lists, the advection launch is
// k_pci_advect_lists, and every solver iteration is two launches over the same lists — A, the predicted density and lambda, and B, the
// position correction into the other predicted-position buffer.  The XSPH launch of the integration stage walks the fluid entries only.
// Each applies the tests of the definition (nrs_kernels_ref.h, "PBF": j != i, length(x_i - x_j) < h at the start positions,
// length(x*_i - x*_j) < h at the predicted ones) and forms the sums in the order of the reference-order walks (one partial per
// (cell, kind) group, fluid before boundary inside a cell), so both paths give the same bits.  The walks themselves are the shared ones
// (nrs_kernels_walk.h); the passes below supply their terms (the term functions of nrs_kernels_ref.h, "PBF").
#pragma once
#include "nrs_kernels_pcisph.h"

namespace nrs {

// ---- iteration launch A: rho*, lambda = -C / (D + eps), e_i --------------------------------------------------------------------------
template <typename R, int KSET> struct PbfLambdaPass {
    typedef R Real;
    typedef typename Vec4T<R>::type T4;
    static constexpr int KS = KSET;
    static constexpr bool WALLED = true;
    Params<R> P;
    PbfArrays<R> A;
    typedef PbfSums<R> Acc;
    struct Own { V3<R> xs1; };
    struct Nb { T4 x; };
    NRS_DEV Own own(uint32_t i, V3<R>) const { return Own{xyz<R>(A.xsIn[i])}; }
    NRS_DEV Acc zero() const { return pbf_zero<R>(); }
    NRS_DEV Acc start(const Own &) const
    {
        Acc t = pbf_zero<R>();
        t.rho += P.particleMass * W_dens<R, KSET>(mk3<R>(0, 0, 0), P.interactionRadius, P.kpoly);
        return t;
    }
    NRS_DEV Nb gather(uint32_t j) const { return Nb{A.xsIn[j]}; }
    NRS_DEV void fluid(const Own &o, V3<R>, const T4 &, const Nb &nb, float, Acc &part) const { pbf_lambda_fluid<R, KSET>(P, o.xs1 - xyz<R>(nb.x), part); }
    NRS_DEV void boundary(const Own &o, V3<R>, uint32_t, const T4 &b, Acc &part) const
    {
        pbf_lambda_boundary<R, KSET>(P, o.xs1 - xyz<R>(b), P.restDensity * b.w, part);
    }
    NRS_DEV void store(uint32_t i, V3<R>, const Own &, const Acc &t) const { pbf_lambda_store<R>(P, A, i, t); }
};

// ---- iteration launch B: dx_i = sum_j (lambda_i + lambda_j) g_ij + sum_b lambda_i g_ib, x* + dx into the other buffer; TENS: with the
// tensile correction s_corr (fluid pairs: lambda_i + lambda_j + s_ij) -----------------------------------------------------------------
template <typename R, int KSET, bool TENS> struct PbfCorrectPass {
    typedef R Real;
    typedef typename Vec4T<R>::type T4;
    static constexpr int KS = KSET;
    static constexpr bool WALLED = true;
    Params<R> P;
    PbfArrays<R> A;
    typename std::conditional<TENS, PbfTensile<R>, WalkUnused>::type T;
    typedef V3<R> Acc;
    struct Own { V3<R> xs1; R li; };
    struct Nb { T4 x; R lj; };
    NRS_DEV Own own(uint32_t i, V3<R>) const { return Own{xyz<R>(A.xsIn[i]), A.lambda[i]}; }
    NRS_DEV Acc zero() const { return mk3<R>(0, 0, 0); }
    NRS_DEV Acc start(const Own &) const { return zero(); }
    NRS_DEV Nb gather(uint32_t j) const { return Nb{A.xsIn[j], A.lambda[j]}; }
    NRS_DEV void fluid(const Own &o, V3<R>, const T4 &, const Nb &nb, float, Acc &part) const
    {
        if constexpr (TENS) part = part + pbf_correct_fluid_s<R, KSET>(P, o.xs1 - xyz<R>(nb.x), o.li, nb.lj, T);
        else part = part + pbf_correct_fluid<R, KSET>(P, o.xs1 - xyz<R>(nb.x), o.li, nb.lj);
    }
    NRS_DEV void boundary(const Own &o, V3<R>, uint32_t, const T4 &b, Acc &part) const
    {
        part = part + pbf_correct_boundary<R, KSET>(P, o.xs1 - xyz<R>(b), P.restDensity * b.w, o.li);
    }
    NRS_DEV void store(uint32_t i, V3<R>, const Own &o, Acc dx) const { pbf_correct_store<R>(A, i, o.xs1, dx); }
};

// ---- the integration stage's fluid-only passes: XSPH (c > 0) and the two launches of the vorticity confinement (eps_v > 0,
// nrs_kernels_ref.h "vorticity confinement").  u = (x* - x) / dt of the particle and of each neighbour ---------------------------------
template <typename R, int KSET> struct PbfFluidPass { // what the three share
    typedef R Real;
    typedef typename Vec4T<R>::type T4;
    static constexpr int KS = KSET;
    static constexpr bool WALLED = false;
    typedef V3<R> Acc;
    NRS_DEV Acc zero() const { return mk3<R>(0, 0, 0); }
    template <typename Own> NRS_DEV Acc start(const Own &) const { return zero(); }
    template <typename Own> NRS_DEV void boundary(const Own &, V3<R>, uint32_t, const T4 &, Acc &) const {}
};
// vel_i = u_i + c sum_j (m / rho0) W (u_j - u_i) (before k_pbf_integrate, which then takes vel as given)
template <typename R, int KSET> struct PbfXsphPass : PbfFluidPass<R, KSET> {
    typedef typename Vec4T<R>::type T4;
    Params<R> P;
    const T4 *__restrict__ xs;
    T4 *__restrict__ vel;
    R c;
    struct Own { V3<R> xs1, v1; };
    struct Nb { T4 x; };
    NRS_DEV Own own(uint32_t i, V3<R> pos1) const { const V3<R> xs1 = xyz<R>(xs[i]); return Own{xs1, pbf_vel<R>(P, xs1, pos1)}; }
    NRS_DEV Nb gather(uint32_t j) const { return Nb{xs[j]}; }
    NRS_DEV void fluid(const Own &o, V3<R>, const T4 &q, const Nb &nb, float, V3<R> &part) const
    {
        const V3<R> xj = xyz<R>(q), xsj = xyz<R>(nb.x);
        part = part + pbf_xsph_fluid<R, KSET>(P, o.xs1 - xsj, pbf_vel<R>(P, xsj, xj), o.v1);
    }
    NRS_DEV void store(uint32_t i, V3<R>, const Own &o, V3<R> sum) const { vel[i] = mk4<R>(o.v1 + pci_scale<R>(c, sum), (R)0.0); }
};
// omega[i] = (omega_i, |omega_i|)
template <typename R, int KSET> struct PbfVorticityPass : PbfFluidPass<R, KSET> {
    typedef typename Vec4T<R>::type T4;
    Params<R> P;
    const T4 *__restrict__ xs;
    T4 *__restrict__ omega;
    struct Own { V3<R> xs1, u1; };
    struct Nb { T4 x; };
    NRS_DEV Own own(uint32_t i, V3<R> pos1) const { const V3<R> xs1 = xyz<R>(xs[i]); return Own{xs1, pbf_vel<R>(P, xs1, pos1)}; }
    NRS_DEV Nb gather(uint32_t j) const { return Nb{xs[j]}; }
    NRS_DEV void fluid(const Own &o, V3<R>, const T4 &q, const Nb &nb, float, V3<R> &part) const
    {
        const V3<R> xj = xyz<R>(q), xsj = xyz<R>(nb.x);
        part = part + pbf_vort_fluid<R, KSET>(P, o.xs1 - xsj, pbf_vel<R>(P, xsj, xj), o.u1);
    }
    NRS_DEV void store(uint32_t i, V3<R>, const Own &, V3<R> sum) const { omega[i] = pbf_vort_pack<R>(sum); }
};
// vel[i] = v_i + dt eps_v (N_i x omega_i), v_i = vel[i] (velGiven: the XSPH launch ran) or u_i
template <typename R, int KSET> struct PbfConfinePass : PbfFluidPass<R, KSET> {
    typedef typename Vec4T<R>::type T4;
    Params<R> P;
    const T4 *__restrict__ xs, *__restrict__ omega;
    T4 *__restrict__ vel;
    int velGiven;
    R epsV;
    struct Own { V3<R> xs1; T4 om; };
    struct Nb { T4 x; R wj; };
    NRS_DEV Own own(uint32_t i, V3<R>) const { return Own{xyz<R>(xs[i]), omega[i]}; }
    NRS_DEV Nb gather(uint32_t j) const { return Nb{xs[j], omega[j].w}; }
    NRS_DEV void fluid(const Own &o, V3<R>, const T4 &, const Nb &nb, float, V3<R> &part) const
    {
        part = part + pbf_eta_fluid<R, KSET>(P, o.xs1 - xyz<R>(nb.x), nb.wj, o.om.w);
    }
    NRS_DEV void store(uint32_t i, V3<R> pos1, const Own &o, V3<R> eta) const
    {
        const V3<R> v = velGiven ? xyz<R>(vel[i]) : pbf_vel<R>(P, o.xs1, pos1);
        vel[i] = mk4<R>(pbf_confine<R>(P, v, eta, o.om, epsV), (R)0.0);
    }
};

} // namespace nrs
