// nrs_kernels_akinci.h — surface tension and wall adhesion of Akinci, Akinci and Teschner (2013) for the PCISPH, PBF and DFSPH
// steps (DESIGN.md "Akinci surface tension and adhesion").
//
// Two launches replace the advection launch of pci_prefix while the model is on (gamma > 0 or beta_a > 0):
//   normals  (gamma > 0 only)  n_i = h sum_j (m / rho_j) grad W(r_ij); one 16-byte record (n_i, rho_i) per sorted slot;
//   advect   the advection launch's own force gather (forces_from_hits / gather_forces, untouched), then ONE more walk that forms
//            S_i = sum_j K_ij ((m C_ij) u_ij + (n_i - n_j))   over the fluid neighbours, K_ij = 2 rho0 / (rho_i + rho_j), u = r / |r|,
//            B_i = sum_b (psi_b A_ib) u_ib                    over the boundary particles,
//            and force_adv = (the existing sum) + ((-gamma m) S_i + (-beta_a m) B_i).
// Fluid neighbours are the j != i with length(r_ij) < h at the sorted start positions; boundary particles are not tested — Aboundary's
// branch is the cut-off.  A pair whose C (A) is exactly 0 adds no cohesion (adhesion) term, so r = 0 never forms 0 * NaN.
// Order of every sum: the 27 cells in z, y, x order, in each cell a fluid partial (j ascending) and then a boundary partial, each added
// to its running total — the order of walk_cells (nrs_kernels_walk.h), which the normals pass uses.  The list-driven kernels (Muller set, plan.lists) form the same partials from
// the hit lists, so both paths give the same bits; a particle whose list overflowed takes the reference-order walk.
#pragma once
#include "nrs_kernels_pcisph.h"

namespace nrs {

template <typename R> struct AkinciView {
    typedef typename Vec4T<R>::type T4;
    T4 *normals; // (n_i, rho_i) per sorted slot; written by the normals launch, read by the advection launch (nullptr while gamma = 0)
    R gamma, beta;
};

// ---- the terms ------------------------------------------------------------------------------------------------------------------------
template <typename R> NRS_DEV V3<R> akinci_unit(V3<R> r, R len) { return mk3<R>(r.x / len, r.y / len, r.z / len); }
// (m / rho_j) grad W(r_ij)
template <typename R, int KSET> NRS_DEV V3<R> akinci_normal_term(const Params<R> &P, V3<R> rij, R rhoj)
{
    return pci_scale<R>(P.particleMass / rhoj, W_grad<R, KSET>(rij, P.interactionRadius, P.kpoly_grad));
}
// K_ij ((m C_ij) u_ij + (n_i - n_j)); nj = the neighbour's record
template <typename R>
NRS_DEV V3<R> akinci_fluid_term(const Params<R> &P, V3<R> rij, V3<R> ni, R rhoi, const typename Vec4T<R>::type &nj)
{
    const R K = ((R)2 * P.restDensity) / (rhoi + nj.w);
    V3<R> t = ni - xyz<R>(nj);
    const R C = Cakinci<R>(rij, P.interactionRadius, P.ksurf1, P.ksurf2);
    if (C != (R)0) t = pci_scale<R>(P.particleMass * C, akinci_unit<R>(rij, (R)length(rij))) + t;
    return pci_scale<R>(K, t);
}
// (psi_b A_ib) u_ib into part (nothing where A = 0)
template <typename R> NRS_DEV void akinci_boundary_term(const Params<R> &P, V3<R> rib, R psi, V3<R> &part)
{
    const R A = Aboundary_clamped<R>(rib, P.interactionRadius, P.bpol);
    if (A != (R)0) part = part + pci_scale<R>(psi * A, akinci_unit<R>(rib, (R)length(rib)));
}
template <typename R> NRS_DEV typename Vec4T<R>::type akinci_normal_pack(const Params<R> &P, V3<R> sum, R rhoi)
{
    return mk4<R>(pci_scale<R>(P.interactionRadius, sum), rhoi);
}
// (-gamma m) S + (-beta_a m) B
template <typename R> NRS_DEV V3<R> akinci_force(const Params<R> &P, const AkinciView<R> &K, V3<R> S, V3<R> B)
{
    return pci_scale<R>(-K.gamma * P.particleMass, S) + pci_scale<R>(-K.beta * P.particleMass, B);
}

// ---- the normals pass (fluid neighbours only): n_i = h sum_j (m / rho_j) grad W(r_ij), stored with rho_i -----------------------------------
template <typename R, int KSET> struct AkinciNormalsPass {
    typedef R Real;
    typedef typename Vec4T<R>::type T4;
    static constexpr int KS = KSET;
    static constexpr bool WALLED = false;
    Params<R> P;
    const R *__restrict__ sDens;
    T4 *__restrict__ normals;
    typedef V3<R> Acc;
    struct Own {};
    struct Nb { R rho; };
    NRS_DEV Own own(uint32_t, V3<R>) const { return Own{}; }
    NRS_DEV Acc zero() const { return mk3<R>(0, 0, 0); }
    NRS_DEV Acc start(const Own &) const { return zero(); }
    NRS_DEV Nb gather(uint32_t j) const { return Nb{sDens[j]}; }
    // (Muller: Wdefault_grad with the length the walk's test formed, which is what W_grad computes again)
    NRS_DEV void fluid(const Own &, V3<R> pos1, const T4 &q, const Nb &nb, float rlen, Acc &part) const
    {
        const V3<R> d = pos1 - xyz<R>(q);
        if constexpr (KSET == KS_MULLER)
            part = part + pci_scale<R>(P.particleMass / nb.rho, Wdefault_grad_len<R>(d, rlen, P.interactionRadius, P.kpoly_grad));
        else part = part + akinci_normal_term<R, KSET>(P, d, nb.rho);
    }
    NRS_DEV void boundary(const Own &, V3<R>, uint32_t, const T4 &, Acc &) const {}
    NRS_DEV void store(uint32_t i, V3<R>, const Own &, Acc sum) const { normals[i] = akinci_normal_pack<R>(P, sum, sDens[i]); }
};

// ---- the force walk, reference order (hand-written: two accumulators) ---------------------------------------------------
// S (when gamma > 0) and B (when beta_a > 0 and HAS_B) of particle i
template <typename R, int KSET, bool HAS_B>
NRS_DEV void akinci_force_walk(const Params<R> &P, const GridView<R> &G, const AkinciView<R> &K,
                               const typename Vec4T<R>::type *__restrict__ sPos, uint32_t i, V3<R> pos1, V3<R> &S, V3<R> &B)
{
    const R ir = P.interactionRadius, rd = P.restDensity;
    const bool coh = K.gamma > (R)0, adh = HAS_B && K.beta > (R)0;
    const I3 gp = calcGridPos<R>(P, pos1);
    V3<R> ni = mk3<R>(0, 0, 0);
    R rhoi = (R)0;
    if (coh) { const typename Vec4T<R>::type own = K.normals[i]; ni = xyz<R>(own); rhoi = own.w; }
    for (int z = -1; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int x = -1; x <= 1; x++) {
                const uint32_t h = calcGridHash<R>(P, gp.x + x, gp.y + y, gp.z + z);
                if (coh) {
                    V3<R> c = mk3<R>(0, 0, 0);
                    const uint32_t s = G.cellStart[h];
                    if (s != CELL_EMPTY) {
                        const uint32_t e = G.cellEnd[h];
                        for (uint32_t j = s; j < e; ++j) {
                            if (j == i) continue;
                            const V3<R> d = pos1 - xyz<R>(sPos[j]);
                            if (length(d) < ir) c = c + akinci_fluid_term<R>(P, d, ni, rhoi, K.normals[j]);
                        }
                    }
                    S = S + c;
                }
                if (HAS_B && adh) {
                    V3<R> cb = mk3<R>(0, 0, 0);
                    const uint32_t sb = G.bCellStart[h];
                    if (sb != CELL_EMPTY) {
                        const uint32_t e = G.bCellEnd[h];
                        for (uint32_t j = sb; j < e; ++j) { // no distance test on boundary particles (as cell_forces)
                            const typename Vec4T<R>::type b = G.sB[j];
                            akinci_boundary_term<R>(P, pos1 - xyz<R>(b), rd * b.w, cb);
                        }
                    }
                    B = B + cb;
                }
            }
}

// the advection launch with the model on: k_pci_advect_ref's gather (SURF: the context's fsurf term, off while gamma > 0) + the walk
template <typename R, int KSET, bool SURF, bool HAS_B>
__global__ __launch_bounds__(BLOCK) void k_akinci_advect_ref(Params<R> P, GridView<R> G, PciArrays<R> A, AkinciView<R> K,
                                                             const typename Vec4T<R>::type *__restrict__ sPos,
                                                             const typename Vec4T<R>::type *__restrict__ sVel,
                                                             const R *__restrict__ sDens, const R *__restrict__ sPres, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const V3<R> pos1 = xyz<R>(sPos[i]), vel1 = xyz<R>(sVel[i]);
    const ForceAcc<R> F = gather_forces<R, KSET, SURF, HAS_B>(P, G, i, pos1, vel1, sDens[i], (R)0.0, sPos, sVel, sDens, sPres);
    V3<R> S = mk3<R>(0, 0, 0), B = mk3<R>(0, 0, 0);
    akinci_force_walk<R, KSET, HAS_B>(P, G, K, sPos, i, pos1, S, B);
    pci_advect_store<R>(P, A, i, pos1, vel1, pci_advect_force<R>(P, F) + akinci_force<R>(P, K, S, B));
}

// ---- list-driven kernels (Muller set) -------------------------------------------------------------------------------------------------
template <typename R, int KSET, bool SURF, bool HAS_B>
NRS_DEV void akinci_advect_lists_particle(const Params<R> &P, const GridView<R> &G, const PciArrays<R> &A, const AkinciView<R> &K,
                                          const HitBuffer &hb, const typename Vec4T<R>::type *__restrict__ sPos,
                                          const typename Vec4T<R>::type *__restrict__ sVel, const R *__restrict__ sDens,
                                          const R *__restrict__ sPres, uint32_t i)
{
    static_assert(KSET == KS_MULLER, "list-driven Akinci kernels: Muller kernels only (the Monaghan support is 2h, Ctx::Features::listKernels)");
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const V3<R> vel1 = xyz<R>(sVel[i]);
    const R pres = (R)0.0;
    const R dens = sDens[i];
    const R ir = P.interactionRadius, rd = P.restDensity;
    const HitCounts hc = unpack_counts(hb.counts[i]);
    ForceAcc<R> F;
    V3<R> S = mk3<R>(0, 0, 0), B = mk3<R>(0, 0, 0);
    if (hc.over) {
        F = gather_forces<R, KSET, SURF, HAS_B>(P, G, i, pos1, vel1, dens, pres, sPos, sVel, sDens, sPres);
        akinci_force_walk<R, KSET, HAS_B>(P, G, K, sPos, i, pos1, S, B);
    } else {
        F = forces_from_hits<R, KSET, SURF, HAS_B, true>(P, G, sPos, sVel, sDens, sPres, pos1, vel1, dens, pres, hb.hits + i, hb.stride, hc, i);
        const bool coh = K.gamma > (R)0, adh = HAS_B && K.beta > (R)0 && hc.nb != 0;
        V3<R> ni = mk3<R>(0, 0, 0);
        R rhoi = (R)0;
        if (coh) { const typename Vec4T<R>::type own = K.normals[i]; ni = xyz<R>(own); rhoi = own.w; }
        if (!adh) { // the fluid entries alone, batched, one partial per cell tag: two 16-byte gathers per neighbour
            if (coh) {
                V3<R> part = mk3<R>(0, 0, 0);
                uint32_t prevTag = 0xffffffffu;
                struct Nb { typename Vec4T<R>::type q, nr; };
                walk_fluid_batched(hb.hits + i, hb.stride, hc.nf, [&](uint32_t j) { return Nb{sPos[j], K.normals[j]}; },
                                   [&](uint32_t j, uint32_t tag, const Nb &nb) {
                                       if (tag != prevTag) { S = S + part; part = mk3<R>(0, 0, 0); prevTag = tag; }
                                       if (j == i) return;
                                       const V3<R> d = pos1 - xyz<R>(nb.q);
                                       if (!(length_listed(dot(d, d)) < ir)) return;
                                       part = part + akinci_fluid_term<R>(P, d, ni, rhoi, nb.nr);
                                   });
                S = S + part;
            }
        } else { // (cell, kind) groups in the reference's order: fluid partials into S, boundary partials into B
            V3<R> part = mk3<R>(0, 0, 0);
            bool partB = false;
            for_each_hit(hb.hits + i, hb.stride, hc, [&](uint32_t j, bool isB, bool fresh) {
                if (fresh) {
                    if (partB) B = B + part; else S = S + part;
                    part = mk3<R>(0, 0, 0);
                    partB = isB;
                }
                if (HAS_B && isB) {
                    const typename Vec4T<R>::type b = G.sB[j];
                    akinci_boundary_term<R>(P, pos1 - xyz<R>(b), rd * b.w, part);
                } else if (coh && j != i) {
                    const V3<R> d = pos1 - xyz<R>(sPos[j]);
                    if (length(d) < ir) part = part + akinci_fluid_term<R>(P, d, ni, rhoi, K.normals[j]);
                }
            });
            if (partB) B = B + part; else S = S + part;
        }
    }
    pci_advect_store<R>(P, A, i, pos1, vel1, pci_advect_force<R>(P, F) + akinci_force<R>(P, K, S, B));
}
template <typename R, int KSET, bool SURF, bool HAS_B, bool WALLS = false>
__global__ __launch_bounds__(BLOCK) void k_akinci_advect_lists(Params<R> P, GridView<R> G, PciArrays<R> A, AkinciView<R> K, HitBuffer hb,
                                                               const typename Vec4T<R>::type *__restrict__ sPos,
                                                               const typename Vec4T<R>::type *__restrict__ sVel,
                                                               const R *__restrict__ sDens, const R *__restrict__ sPres, uint32_t n,
                                                               WallList wl, uint32_t wallBlocks)
{
    wall_split<HAS_B, WALLS>(hb, wl, wallBlocks, n, [&](auto hasB, uint32_t i) {
        akinci_advect_lists_particle<R, KSET, SURF, decltype(hasB)::value>(P, G, A, K, hb, sPos, sVel, sDens, sPres, i);
    });
}

} // namespace nrs
