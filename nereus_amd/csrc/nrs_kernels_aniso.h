// nrs_kernels_aniso.h — the two kernels of the anisotropic surface reconstruction (include/nereus_hip.h "anisotropic surface
// reconstruction"; DESIGN.md "Anisotropic kernels"): k_aniso_records, pass A, one thread per sorted particle, and k_aniso_lattice, pass B,
// one thread per lattice node.  Both walk the 5 x 5 x 5 unwrapped cell neighbourhood of their owner in the sampler's fluid cell table
// (FieldSampler, nrs_field_sampler.h): cells z, y, x ascending, sorted slots ascending, one accumulator per component — the order is
// part of the interface; the five cells of an x-row are walked as one run of sorted slots, which keeps it.  The terms and the finishing
// routine are nrs_host_aniso.h's.  No atomics, no LDS, vector stores only.
#pragma once
#include "nrs_host_aniso.h"
#include "nrs_kernels_sample.h"

namespace nrs {

// One run of sorted slots: the cells h0 .. h0 + cnt - 1 are consecutive hashes, so their particles are consecutive sorted slots, from the
// start of the first cell that has any to the end of the last; f(j) for every slot j, ascending
template <typename R, typename F> NRS_DEV void aniso_run(const GridView<R> &G, uint32_t h0, uint32_t cnt, F &&f)
{
    uint32_t a = 0, s = CELL_EMPTY;
    for (; a < cnt; ++a) {
        s = G.cellStart[h0 + a];
        if (s != CELL_EMPTY) break;
    }
    if (s == CELL_EMPTY) return;
    uint32_t b = cnt - 1;
    for (; b > a; --b)
        if (G.cellStart[h0 + b] != CELL_EMPTY) break;
    const uint32_t e = G.cellEnd[h0 + b];
    if (!run_ok<R>(G, s, e)) return;
    for (uint32_t j = s; j < e; ++j) f(j);
}
// The 5 x 5 x 5 unwrapped cell neighbourhood of the cell gp: rows z, y ascending; the five cells of an x-row as one run of sorted
// slots, split where the row wraps (gridSize >= 8: the two parts do not meet).  Unsigned sums: an owner far outside the grid has
// saturated cell coordinates, and only their low bits count.
template <typename R, typename F> NRS_DEV void aniso_walk(const Params<R> &P, const GridView<R> &G, I3 gp, F &&f)
{
    const uint32_t nx = P.gridSize[0];
    const uint32_t x0 = grid_x<R>(P, (int)((uint32_t)gp.x - 2u));
    const uint32_t n1 = nx - x0 < 5u ? nx - x0 : 5u; // cells of the row before the wrap
    for (int z = -2; z <= 2; z++)
        for (int y = -2; y <= 2; y++) {
            // (the hash of the row's cell with x = 0: grid_x of the window's first column)
            const uint32_t row = calcGridHash<R>(P, (int)P.numBodies, (int)((uint32_t)gp.y + (uint32_t)y), (int)((uint32_t)gp.z + (uint32_t)z));
            aniso_run<R>(G, row + x0, n1, f);
            if (n1 < 5u) aniso_run<R>(G, row, 5u - n1, f);
        }
}

// where pass A stores
template <typename R> struct AnisoOut {
    typedef typename Vec4T<R>::type T4;
    T4 *center; // [n]  centre, bound
    T4 *g;      // [2n] (G00, G01, G02, G11), (G12, G22, weight, 0)
    uint32_t *count, *index;
};

// Pass A.  sPos: the sampler's sorted positions, sIndex: its sort values (the particle's index in download order).
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_aniso_records(Params<R> P, GridView<R> G, AnisoConsts<R> K, const typename Vec4T<R>::type *__restrict__ sPos,
                                                         const uint32_t *__restrict__ sIndex, AnisoOut<R> O, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const V3<R> x = xyz<R>(sPos[i]);
    AnisoSums<R> S = aniso_sums_zero<R>();
    if (finite3<R>(x)) {
        const I3 gp = calcGridPos<R>(P, x);
        aniso_walk<R>(P, G, gp, [&](uint32_t j) {
            const V3<R> xj = xyz<R>(sPos[j]);
            aniso_add_neighbour<R>(K, S, xj.x - x.x, xj.y - x.y, xj.z - x.z);
        });
    }
    const AnisoRecord<R> A = aniso_finish<R>(K, x.x, x.y, x.z, S);
    O.center[i] = mk4<R>(A.cx, A.cy, A.cz, A.bound);
    O.g[2 * (size_t)i] = mk4<R>(A.g00, A.g01, A.g02, A.g11);
    O.g[2 * (size_t)i + 1] = mk4<R>(A.g12, A.g22, A.weight, (R)0);
    O.count[i] = S.count;
    O.index[i] = sIndex[i];
}

// Pass B.  Node q of the lattice L (linear index (k * dims[1] + j) * dims[0] + i) is formed here.  center / g: pass A's records; sVel: the
// sampler's sorted velocities.  dens is always written; grad / vel unless null.  Only the first test of a candidate needs its first
// record: most candidates leave after one 16- or 32-byte load.
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_aniso_lattice(Params<R> P, GridView<R> G, const typename Vec4T<R>::type *__restrict__ center,
                                                         const typename Vec4T<R>::type *__restrict__ g, const typename Vec4T<R>::type *__restrict__ sVel,
                                                         Lattice L, R *__restrict__ dens, typename Vec4T<R>::type *__restrict__ grad,
                                                         typename Vec4T<R>::type *__restrict__ vel, uint32_t m)
{
    typedef typename Vec4T<R>::type T4;
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= m) return;
    const uint32_t li = q % L.dims[0], lt = q / L.dims[0];
    const V3<R> x = lattice_node<R>(L, li, lt % L.dims[1], lt / L.dims[1]);
    R phi = (R)0;
    V3<R> gr = mk3<R>(0, 0, 0), vn = mk3<R>(0, 0, 0);
    if (finite3<R>(x) && G.nSorted) {
        const I3 gp = calcGridPos<R>(P, x);
        aniso_walk<R>(P, G, gp, [&](uint32_t j) {
            const T4 cj = center[j];
            const R dx = x.x - cj.x, dy = x.y - cj.y, dz = x.z - cj.z;
            const R d2 = (dx * dx + dy * dy) + dz * dz;
            if (!(d2 < cj.w * cj.w)) return;
            const T4 ga = g[2 * (size_t)j], gb = g[2 * (size_t)j + 1];
            // G = (ga.x ga.y ga.z; ga.y ga.w gb.x; ga.z gb.x gb.y)
            const R g0 = (ga.x * dx + ga.y * dy) + ga.z * dz;
            const R g1 = (ga.y * dx + ga.w * dy) + gb.x * dz;
            const R g2 = (ga.z * dx + gb.x * dy) + gb.y * dz;
            const R q2 = (g0 * g0 + g1 * g1) + g2 * g2;
            if (!(q2 < (R)1)) return;
            const R p = (R)1 - q2;
            const R wp2 = gb.z * (p * p);
            const R t = wp2 * p;
            phi += t;
            if (grad) {
                const R f = (R)-6 * wp2;
                gr.x += f * ((ga.x * g0 + ga.y * g1) + ga.z * g2);
                gr.y += f * ((ga.y * g0 + ga.w * g1) + gb.x * g2);
                gr.z += f * ((ga.z * g0 + gb.x * g1) + gb.y * g2);
            }
            if (vel) {
                const T4 vj = sVel[j];
                vn.x += t * vj.x; vn.y += t * vj.y; vn.z += t * vj.z;
            }
        });
    }
    dens[q] = phi;
    if (grad) grad[q] = mk4<R>(gr, (R)0);
    if (vel) vel[q] = phi != (R)0 ? mk4<R>(vn.x / phi, vn.y / phi, vn.z / phi, phi) : mk4<R>((R)0, (R)0, (R)0, (R)0);
}

} // namespace nrs
