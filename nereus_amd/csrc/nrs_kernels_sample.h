// nrs_kernels_sample.h — the field sampler's gather (include/nereus_hip.h "field sampling"; DESIGN.md "Field sampling"): the SPH sums
// of the solvers evaluated at positions that are not particles.  The owners of the sums are queries — caller-supplied points, or the
// nodes of a lattice formed on the device —, the candidates the sampler's own sorted copy of the fluid (FieldSampler,
// nrs_field_sampler.h) and, for NRS_FIELD_WALLS, the context's sorted boundary particles.
//
// The terms are the solvers' (nrs_math.h: the cut-off test of density_of, W_dens, W_grad, the float scalar operand of scalar x vector,
// SURVEY Q11).  The ORDER of every sum is part of the interface: one accumulator per output component; the 27 cells of the query's
// unwrapped neighbourhood z, y, x ascending; in a cell the sorted slots ascending; with walls a cell's boundary particles after its
// fluid particles.
#pragma once
#include "nrs_host_sample.h"
#include "nrs_kernels_ref.h"

namespace nrs {

// node (i, j, k) of a lattice (Lattice, nrs_host_sample.h): (R)(origin + idx * spacing), product and sum in double, one rounding to R
template <typename R> NRS_DEV V3<R> lattice_node(const Lattice &L, uint32_t i, uint32_t j, uint32_t k)
{
    return mk3<R>((R)(L.origin[0] + (double)i * L.spacing[0]), (R)(L.origin[1] + (double)j * L.spacing[1]), (R)(L.origin[2] + (double)k * L.spacing[2]));
}

// where the results of a call go; a null pointer: not asked for
template <typename R> struct SampleOut {
    typedef typename Vec4T<R>::type T4;
    R *dens;
    T4 *grad, *vel;
    uint32_t *count;
};

// the accumulators of one query
template <typename R> struct SampleAcc {
    R dens, wsum;       // rho (with the wall terms, if asked for); the fluid-only sum of m W: the Shepard denominator
    V3<R> grad, vnum;   // grad rho; sum (m W_j) v_j
    uint32_t count;
};
template <typename R> NRS_DEV SampleAcc<R> sample_acc_zero()
{
    SampleAcc<R> A;
    A.dens = A.wsum = (R)0;
    A.grad = A.vnum = mk3<R>(0, 0, 0);
    A.count = 0u;
    return A;
}

// one fluid candidate at xj for the query at x; vel(): the candidate's velocity, asked for only when a velocity term is formed
template <typename R, int KSET, typename Vel>
NRS_DEV void sample_fluid_term(const Params<R> &P, uint32_t fields, SampleAcc<R> &A, V3<R> x, V3<R> xj, Vel &&vel)
{
    const R ir = P.interactionRadius, pm = P.particleMass;
    const V3<R> d = x - xj;
    const float len = length(d);
    if (len < ir) {
        ++A.count;
        const R w = pm * W_dens<R, KSET>(d, ir, P.kpoly);
        A.dens += w;
        A.wsum += w;
        // (Wmonaghan_grad is 0 / 0 at length 0, and lattice nodes do coincide with particles: such a neighbour has no gradient term)
        if ((fields & NRS_FIELD_GRADIENT) && len != 0.0f) A.grad = A.grad + (pm * W_grad<R, KSET>(d, ir, P.kpoly_grad));
        if (fields & NRS_FIELD_VELOCITY) A.vnum = A.vnum + (w * vel());
    }
}
// one boundary candidate b (xyz + V_b in w): the wall term of density_of
template <typename R, int KSET> NRS_DEV void sample_wall_term(const Params<R> &P, SampleAcc<R> &A, V3<R> x, const typename Vec4T<R>::type &b)
{
    const R ir = P.interactionRadius;
    const V3<R> d = x - xyz<R>(b);
    if (length(d) < ir) {
        const R psi = P.restDensity * b.w;
        A.dens += (psi * W_dens<R, KSET>(d, ir, P.kpoly));
    }
}

template <typename R> NRS_DEV bool finite3(V3<R> x) { return isfinite(x.x) && isfinite(x.y) && isfinite(x.z); }

// The per-query walk: the semantic definition of every field.  x is finite.  G: the sampler's fluid cell table (cellStart / cellEnd,
// nSorted, err) and, with HAS_B and walls, the context's boundary tables (bCellStart / bCellEnd / sB).
template <typename R, int KSET, bool HAS_B>
NRS_DEV SampleAcc<R> sample_walk(const Params<R> &P, const GridView<R> &G, const typename Vec4T<R>::type *__restrict__ sPos,
                                 const typename Vec4T<R>::type *__restrict__ sVel, V3<R> x, uint32_t fields)
{
    SampleAcc<R> A = sample_acc_zero<R>();
    const I3 gp = calcGridPos<R>(P, x);
    const bool walls = HAS_B && (fields & NRS_FIELD_WALLS);
    for (int z = -1; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int c = -1; c <= 1; c++) {
                // (unsigned sums: a query far outside the grid has saturated cell coordinates, and only their low bits count)
                const uint32_t h = calcGridHash<R>(P, (int)((uint32_t)gp.x + (uint32_t)c), (int)((uint32_t)gp.y + (uint32_t)y), (int)((uint32_t)gp.z + (uint32_t)z));
                const uint32_t s = G.cellStart[h];
                if (s != CELL_EMPTY) {
                    const uint32_t e = G.cellEnd[h];
                    if (run_ok<R>(G, s, e))
                        for (uint32_t j = s; j < e; ++j) sample_fluid_term<R, KSET>(P, fields, A, x, xyz<R>(sPos[j]), [&] { return xyz<R>(sVel[j]); });
                }
                if (walls) {
                    const uint32_t sb = G.bCellStart[h];
                    if (sb != CELL_EMPTY) {
                        const uint32_t eb = G.bCellEnd[h];
                        for (uint32_t j = sb; j < eb; ++j) sample_wall_term<R, KSET>(P, A, x, G.sB[j]);
                    }
                }
            }
    return A;
}

// the stores of one query; ok == false: a query with a non-finite coordinate (zeros, count 0)
template <typename R> NRS_DEV void sample_store(const SampleOut<R> &O, uint32_t q, bool ok, const SampleAcc<R> &A)
{
    if (O.dens) O.dens[q] = ok ? A.dens : (R)0;
    if (O.grad) O.grad[q] = ok ? mk4<R>(A.grad, (R)0) : mk4<R>((R)0, (R)0, (R)0, (R)0);
    if (O.vel) {
        const bool some = ok && A.wsum != (R)0;
        O.vel[q] = some ? mk4<R>(A.vnum.x / A.wsum, A.vnum.y / A.wsum, A.vnum.z / A.wsum, A.wsum) : mk4<R>((R)0, (R)0, (R)0, (R)0);
    }
    if (O.count) O.count[q] = ok ? A.count : 0u;
}

// One thread per query.  points: the m positions of nrs_sample_points; null: query q is node q of the lattice L (linear index
// (k * dims[1] + j) * dims[0] + i), formed here.  fields selects the terms that are formed; O the stores.  It serves both entry points:
// a kernel that gave a 4 x 4 x 4 brick of nodes to one wavefront and streamed the brick's hull of cells to all lanes lost the A/B
// against this walk on the lattice and was deleted (DESIGN.md "Field sampling" has the numbers and the reason).
template <typename R, int KSET, bool HAS_B>
__global__ __launch_bounds__(BLOCK) void k_sample_points(Params<R> P, GridView<R> G, const typename Vec4T<R>::type *__restrict__ sPos,
                                                         const typename Vec4T<R>::type *__restrict__ sVel,
                                                         const typename Vec4T<R>::type *__restrict__ points, Lattice L,
                                                         SampleOut<R> O, uint32_t fields, uint32_t m)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= m) return;
    V3<R> x;
    if (points) {
        x = xyz<R>(points[q]);
    } else {
        const uint32_t i = q % L.dims[0], t = q / L.dims[0];
        x = lattice_node<R>(L, i, t % L.dims[1], t / L.dims[1]);
    }
    const bool ok = finite3<R>(x);
    SampleAcc<R> A = sample_acc_zero<R>();
    if (ok && G.nSorted) A = sample_walk<R, KSET, HAS_B>(P, G, sPos, sVel, x, fields);
    sample_store<R>(O, q, ok, A);
}

} // namespace nrs
