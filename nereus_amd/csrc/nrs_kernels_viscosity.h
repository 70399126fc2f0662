// nrs_kernels_viscosity.h — the kernels of the implicit viscosity solve of the DFSPH step (DESIGN.md "Implicit viscosity";
// the host decisions and the contract: nrs_host_viscosity.h; the owner: nrs_viscosity.h).
//
// (A u)_i = u_i - dt nu   (rho0 / rho_i) 10 sum_j (rho0 / rho_j) ((u_i - u_j) . x_ij) / (|x_ij|^2 + 0.01 h^2) g_ij
//               - dt nu_b (rho0 / rho_i) 10 sum_b                ( u_i        . x_ib) / (|x_ib|^2 + 0.01 h^2) g_ib
// at the step's start positions, with DFSPH's neighbour rule and gradients (nrs_kernels_ref.h "DFSPH") and rho of the step's scan.  The
// matvec is one neighbour pass (nrs_kernels_walk.h): both kernel paths, the wall workgroups, the overflow fallback and the order of
// summation are the walk's, so the list kernels and the reference-order kernels give the same bits.  The two vector kernels form
// alpha and beta themselves from the reduced sums (device doubles, nrs_host_viscosity.h): no host wait lies inside an iteration.
#pragma once
#include "nrs_host_viscosity.h"
#include "nrs_kernels_dfsph.h"

namespace nrs {

template <typename R> struct ViscArrays {
    typedef typename Vec4T<R>::type T4;
    const T4 *in;  // what the operator is applied to: b = vel_adv in the first launch, p afterwards
    const R *dens; // rho of the step's density scan
    T4 *r, *p, *q; // the first launch writes r = p = b - A b, the later ones q = A p
    R *dotA, *dotB; // per particle: the first launch r_i . r_i and b_i . b_i, the later ones p_i . q_i
    R cF, cB;      // 10 dt nu, 10 dt nu_b
};
// the term of one neighbour at separation d: c ((u_i - u_j) . d) / (|d|^2 + 0.01 h^2) g, with c = 10 dt nu rho0 / rho_j (a wall: 10 dt nu_b)
template <typename R> NRS_DEV R visc_coef(const Params<R> &P, V3<R> d, V3<R> du, R c)
{
    const R h = P.interactionRadius;
    return c * pbf_dot<R>(du, d) / (pbf_dot<R>(d, d) + (R)0.01 * h * h);
}

template <typename R, int KSET, bool START> struct ViscMatvecPass {
    typedef R Real;
    typedef typename Vec4T<R>::type T4;
    static constexpr int KS = KSET;
    static constexpr bool WALLED = true;
    Params<R> P;
    ViscArrays<R> A;
    typedef V3<R> Acc;
    struct Own { V3<R> p; R rho; };
    struct Nb { T4 p; R rho; };
    NRS_DEV Own own(uint32_t i, V3<R>) const { return Own{xyz<R>(A.in[i]), A.dens[i]}; }
    NRS_DEV Acc zero() const { return mk3<R>(0, 0, 0); }
    NRS_DEV Acc start(const Own &) const { return zero(); }
    NRS_DEV Nb gather(uint32_t j) const { return Nb{A.in[j], A.dens[j]}; }
    NRS_DEV void fluid(const Own &o, V3<R> pos1, const T4 &q, const Nb &nb, float, Acc &part) const
    {
        const V3<R> d = pos1 - xyz<R>(q);
        const R c = visc_coef<R>(P, d, o.p - xyz<R>(nb.p), A.cF * (P.restDensity / nb.rho));
        part = part + pci_scale<R>(c, dfsph_g<R, KSET>(P, d, P.particleMass));
    }
    NRS_DEV void boundary(const Own &o, V3<R> pos1, uint32_t, const T4 &b, Acc &part) const
    {
        const V3<R> d = pos1 - xyz<R>(b);
        const R c = visc_coef<R>(P, d, o.p, A.cB);
        part = part + pci_scale<R>(c, dfsph_g<R, KSET>(P, d, P.restDensity * b.w));
    }
    NRS_DEV void store(uint32_t i, V3<R>, const Own &o, const Acc &t) const
    {
        const V3<R> Ap = o.p - pci_scale<R>(P.restDensity / o.rho, t);
        if constexpr (START) {
            const V3<R> r = o.p - Ap;
            const T4 r4 = mk4<R>(r, (R)0.0);
            A.r[i] = r4;
            A.p[i] = r4;
            A.dotA[i] = pbf_dot<R>(r, r);
            A.dotB[i] = pbf_dot<R>(o.p, o.p);
        } else {
            A.q[i] = mk4<R>(Ap, (R)0.0);
            A.dotA[i] = pbf_dot<R>(o.p, Ap);
        }
    }
};

// u += alpha p, r -= alpha q, alpha = rr / (p.q) (visc_alpha), and r_i . r_i for the next rr.  scal: the solve's device scalars; rrSlot:
// where this iteration's rr is.  alpha = 0 leaves u and r as they are, bit for bit.  One thread counts the iteration if it began with rr > 0.
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_visc_update(double *__restrict__ scal, int rrSlot, typename Vec4T<R>::type *__restrict__ u,
                                                       typename Vec4T<R>::type *__restrict__ r, const typename Vec4T<R>::type *__restrict__ p,
                                                       const typename Vec4T<R>::type *__restrict__ q, R *__restrict__ dot, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const double rr = scal[rrSlot];
    const double alpha = visc_alpha(rr, scal[VISC_PQ]);
    if (i == 0 && rr > 0.0) scal[VISC_ITERS] += 1.0;
    if (i >= n) return;
    typename Vec4T<R>::type ri = r[i];
    if (alpha != 0.0) {
        const R a = (R)alpha;
        const typename Vec4T<R>::type ui = u[i];
        u[i] = mk4<R>(xyz<R>(ui) + pci_scale<R>(a, xyz<R>(p[i])), ui.w);
        ri = mk4<R>(xyz<R>(ri) - pci_scale<R>(a, xyz<R>(q[i])), (R)0.0);
        r[i] = ri;
    }
    dot[i] = pbf_dot<R>(xyz<R>(ri), xyz<R>(ri));
}
// p = r + beta p, beta = rr' / rr (visc_beta)
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_visc_direction(const double *__restrict__ scal, int rrSlot, int rrNewSlot,
                                                          typename Vec4T<R>::type *__restrict__ p, const typename Vec4T<R>::type *__restrict__ r,
                                                          uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const R b = (R)visc_beta(scal[rrNewSlot], scal[rrSlot]);
    p[i] = mk4<R>(xyz<R>(r[i]) + pci_scale<R>(b, xyz<R>(p[i])), (R)0.0);
}

} // namespace nrs
