// nrs_kernels_ref.h — "reference-order" gfx950 kernels for the SPH step.
//
// One thread per SORTED slot (coalesced own loads/stores; the reference's thread→slot indirection
// through gridParticleIndex is dropped), the 27 neighbour cells walked z,y,x with j ascending
// and one partial sum per cell, i.e. every floating-point sum is formed in the order the reference forms
// it.  Selected with NRS_FLAG_REFERENCE_ORDER; used for bit-level comparison with the oracle and as the
// semantic definition the tiled kernels (nrs_kernels_tiled.h) are checked against.
//
// What each kernel computes is specified by the reference kernel cited above it.  The physics statements of the force /
// density / IISPH loops (and the smoothing kernels of nrs_math.h) are restatements of the reference's expressions IN THE
// REFERENCE'S EVALUATION ORDER (the local names are this build's own; the oracle keeps the reference's for line-by-line reading): the parity goal
// (every float sum bit-identical to the reference's arithmetic) forces the expression order; everything around them —
// thread mapping, memory layout, templates, boundary packing, double-buffered P_l — is this build's own.
#pragma once
#include "nrs_math.h"
#include <climits>

namespace nrs {

template <typename R> struct GridView {
    typedef typename Vec4T<R>::type T4;
    const uint32_t *cellStart, *cellEnd;   // fluid cell table
    const uint32_t *bCellStart, *bCellEnd; // boundary cell table (valid only when the kernel has HAS_B)
    const T4 *sB;                          // sorted boundary particles: xyz + Vbi in w
    // slab decomposition: a gather kernel evaluates only particles whose (unwrapped) cell-x is in [actLo, actHi)
    // and writes zeros for the rest (halo copies whose neighbourhood is incomplete on this rank)
    int actLo, actHi;
    // consistency guard of the production scans: a fluid run [a, b) read from the cell table must lie inside the sorted array
    // (b >= a, b <= nSorted).  A table built from a wrongly sized merge breaks that, and an unguarded sweep then walks off the
    // allocation (the GPU memory fault of round 1); a run that fails the test is skipped and *err is set — the host reports
    // NRS_E_STATE at the next nrs_synchronize / nrs_download instead of the device faulting.
    uint32_t nSorted;
    uint32_t *err;
    // compact scan candidates (nrs_math.h, quantize_pos): one word per sorted slot, written by the reorder kernels; qT = integer
    // squared-distance threshold of the superset test; null = this context scans the exact positions
    const qword_t *qpos;
    uint32_t qT;
    QuantCfg qc;
};
template <typename R> NRS_DEV bool run_ok(const GridView<R> &G, uint32_t a, uint32_t b)
{
    const bool ok = (b >= a) & (b <= G.nSorted);
    if (!ok && G.err) *G.err = 1u;
    return ok;
}

template <typename R> NRS_DEV bool slab_active(const Params<R> &P, const GridView<R> &G, R x)
{
    // (a single-domain context has no inactive range: without the first test a particle with x = +inf — its cell index saturates past
    // INT_MAX — would be skipped, where the reference gives it its self term; found by the randomised soak against the oracle, round 3)
    if (G.actLo == INT_MIN) return true;
    const long long cx = (long long)floor((x - P.worldOrigin[0]) / P.cellSize[0]);
    return cx >= (long long)G.actLo && cx < (long long)G.actHi;
}

// ---- calcHashD (sph_kernel_impl.cuh:127-145) -------------------------------------------------------
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_hash(Params<R> P, const typename Vec4T<R>::type *__restrict__ pos,
                                                uint32_t *__restrict__ hash, uint32_t *__restrict__ index, uint32_t n)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    I3 g = calcGridPos<R>(P, xyz<R>(pos[i]));
    hash[i] = calcGridHash<R>(P, g.x, g.y, g.z);
    index[i] = i;
}

// Wall particles (see k_density_tiled, nrs_kernels_tiled.h): a sorted slot whose cell is flagged "some boundary particle in the
// 27-neighbourhood" in this static bit table is evaluated by the wall workgroups of the gather launches.
struct WallList {
    const uint32_t *nearBits; // bit per cell
    const uint32_t *hash;     // sorted keys of the step (the cell of every slot)
    const uint32_t *list;     // this step's wall slots, ascending
    const uint32_t *count;    // how many
    const unsigned long long *mask; // bit per sorted slot (one word per wavefront of the reorder kernel): is it a wall slot
};
// Wall slots per 256-slot tile, counted by the reorder kernels while they have each slot's key in a register (first step of the
// wall-list build: counts -> k_resort_scan_tiles -> k_wall_compact).  Called by EVERY thread of the block (it has a barrier);
// h is ignored when !live.
// forceWall: the slot goes to the wall workgroups whatever its cell (an owner the quantised scan cannot serve, see quant_far).
NRS_DEV void wall_tile_count(const uint32_t *__restrict__ nearBits, uint32_t *__restrict__ tileCount, uint32_t h, bool live,
                             unsigned long long *__restrict__ slotMask, bool forceWall = false)
{
    __shared__ uint32_t wallWaveCnt[256 / 64];
    const bool take = live && (forceWall || ((nearBits[h >> 5] >> (h & 31u)) & 1u));
    const unsigned long long m = __ballot(take);
    if ((threadIdx.x & 63u) == 0) {
        wallWaveCnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
        slotMask[(blockIdx.x * 256u + threadIdx.x) >> 6] = m; // (the wall-list compaction and the interior workgroups read this instead of the keys)
    }
    __syncthreads();
    if (threadIdx.x == 0) tileCount[blockIdx.x] = wallWaveCnt[0] + wallWaveCnt[1] + wallWaveCnt[2] + wallWaveCnt[3];
}

// ---- reorderDataAndFindCellStartD (sph_kernel_impl.cuh:210-281) -------------------------------------
// cellStart must have been filled with 0xff.  Also emits inv[index[i]] = i (needed for SURVEY Q5).
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_reorder(const uint32_t *__restrict__ hash, const uint32_t *__restrict__ index,
                                                   const typename Vec4T<R>::type *__restrict__ oldPos,
                                                   const typename Vec4T<R>::type *__restrict__ oldVel,
                                                   const R *__restrict__ oldPres,
                                                   typename Vec4T<R>::type *__restrict__ sPos,
                                                   typename Vec4T<R>::type *__restrict__ sVel, R *__restrict__ sPres,
                                                   uint32_t *__restrict__ cellStart, uint32_t *__restrict__ cellEnd,
                                                   uint32_t *__restrict__ inv, uint32_t n,
                                                   const uint32_t *__restrict__ nearBits, uint32_t *__restrict__ wallTileCount,
                                                   unsigned long long *__restrict__ wallMask, QuantCfg qc, qword_t *__restrict__ qpos)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t src = 0u;
    typename Vec4T<R>::type p4 = mk4<R>((R)0, (R)0, (R)0, (R)0);
    if (i < n) { src = index[i]; p4 = oldPos[src]; }
    // owners outside the range of the quantised scan (too far from the grid origin, NaN) are handed to the wall workgroups, whose
    // scan reads exact positions
    if (nearBits) wall_tile_count(nearBits, wallTileCount, i < n ? hash[i] : 0u, i < n, wallMask, qpos && quant_far<R>(qc, xyz<R>(p4)));
    if (i >= n) return;
    const uint32_t h = hash[i];
    if (i == 0) {
        cellStart[h] = 0;
    } else {
        const uint32_t hp = hash[i - 1];
        if (h != hp) { cellStart[h] = i; cellEnd[hp] = i; }
    }
    if (i == n - 1) cellEnd[h] = n;
    sPos[i] = p4;
    if (qpos) qpos[i] = quantize_pos<R>(qc, xyz<R>(p4));
    sVel[i] = oldVel[src];
    if (oldPres) sPres[i] = oldPres[src];
    if (inv) inv[src] = i;
}

// Undo of the cell table after a step: reset cellStart of exactly the cells the step filled (replaces the
// reference's per-step cudaMemset of 4*numCells bytes, sph_cuda.cu:318, whose cost grows with the EMPTY volume)
static __global__ __launch_bounds__(BLOCK) void k_clear_cells(const uint32_t *__restrict__ hash, uint32_t *__restrict__ cellStart,
                                                       uint32_t n)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = hash[i];
    if (i == 0 || h != hash[i - 1]) cellStart[h] = CELL_EMPTY;
}

// boundary flavour (sph_kernel_impl.cuh:150-205, intended semantics — SURVEY Q1): sorted xyz + vbi packed in one vec4
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_reorder_boundary(const uint32_t *__restrict__ hash,
                                                            const uint32_t *__restrict__ index,
                                                            const typename Vec4T<R>::type *__restrict__ bi,
                                                            const R *__restrict__ vbi,
                                                            typename Vec4T<R>::type *__restrict__ sB,
                                                            uint32_t *__restrict__ cellStart,
                                                            uint32_t *__restrict__ cellEnd, uint32_t n)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = hash[i];
    if (i == 0) {
        cellStart[h] = 0;
    } else {
        const uint32_t hp = hash[i - 1];
        if (h != hp) { cellStart[h] = i; cellEnd[hp] = i; }
    }
    if (i == n - 1) cellEnd[h] = n;
    const uint32_t src = index[i];
    typename Vec4T<R>::type b = bi[src];
    b.w = vbi[src];
    sB[i] = b;
}

// ---- density sum shared by computeDensityPressure (:365-433) and computeIisphDensity (:770-846) ----
template <typename R, int KSET, bool HAS_B>
NRS_DEV R density_of(const Params<R> &P, const GridView<R> &G, const typename Vec4T<R>::type *__restrict__ sPos,
                     uint32_t self)
{
    const V3<R> p = xyz<R>(sPos[self]);
    const I3 gp = calcGridPos<R>(P, p);
    const R ir = P.interactionRadius, kp = P.kpoly, pm = P.particleMass, rd = P.restDensity;
    R dens = (R)0.0;
    dens += pm * W_dens<R, KSET>(mk3<R>(0, 0, 0), ir, kp);
    for (int z = -1; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int x = -1; x <= 1; x++) {
                const uint32_t h = calcGridHash<R>(P, gp.x + x, gp.y + y, gp.z + z);
                {
                    R c = (R)0.0;
                    const uint32_t s = G.cellStart[h];
                    if (s != CELL_EMPTY) {
                        const uint32_t e = G.cellEnd[h];
                        for (uint32_t j = s; j < e; ++j) {
                            if (j != self) {
                                const V3<R> d = p - xyz<R>(sPos[j]);
                                if (length(d) < ir) c += (pm * W_dens<R, KSET>(d, ir, kp));
                            }
                        }
                    }
                    dens += c;
                }
                if (HAS_B) {
                    R c = (R)0.0;
                    const uint32_t s = G.bCellStart[h];
                    if (s != CELL_EMPTY) {
                        const uint32_t e = G.bCellEnd[h];
                        for (uint32_t j = s; j < e; ++j) {
                            const typename Vec4T<R>::type b = G.sB[j];
                            const V3<R> d = p - xyz<R>(b);
                            if (length(d) < ir) {
                                const R psi = rd * b.w;
                                c += (psi * W_dens<R, KSET>(d, ir, kp));
                            }
                        }
                    }
                    dens += c;
                }
            }
    return dens;
}

// Tait equation of state (sph_kernel_impl.cuh:426)
template <typename R> NRS_DEV R tait_pressure(const Params<R> &P, R dens)
{
    return P.gasStiffness * (pow7f((float)(dens / P.restDensity)) - 1);
}

template <typename R, int KSET, bool HAS_B>
__global__ __launch_bounds__(BLOCK) void k_density_ref(Params<R> P, GridView<R> G,
                                                       const typename Vec4T<R>::type *__restrict__ sPos,
                                                       R *__restrict__ dens, R *__restrict__ pres, uint32_t n)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (!slab_active<R>(P, G, sPos[i].x)) { dens[i] = (R)0; if (pres) pres[i] = (R)0; return; }
    const R d = density_of<R, KSET, HAS_B>(P, G, sPos, i);
    dens[i] = d;
    if (pres) pres[i] = tait_pressure<R>(P, d);
}

// ---- computeCellForces (sph_kernel_impl.cuh:442-604) -------------------------------------------------
template <typename R> struct ForceAcc { V3<R> fpres, fvisc, fsurf, fbound; };

template <typename R, int KSET, bool SURF, bool HAS_B>
NRS_DEV void cell_forces(const Params<R> &P, const GridView<R> &G, ForceAcc<R> &A, uint32_t h, uint32_t self,
                         V3<R> pos1, V3<R> vel1, R dens, R pres, const typename Vec4T<R>::type *__restrict__ sPos,
                         const typename Vec4T<R>::type *__restrict__ sVel, const R *__restrict__ sDens,
                         const R *__restrict__ sPres)
{
    const R pm = P.particleMass, m2 = P.particleMass, ir = P.interactionRadius, kp = P.kpoly;
    const R kappa = P.surfaceTension;
    const R kprg = P.kpress_grad, kvg = P.kvisc_grad, kvd = P.kvisc_denum;
    uint32_t s = G.cellStart[h];
    if (s != CELL_EMPTY) {
        const uint32_t e = G.cellEnd[h];
        for (uint32_t j = s; j < e; ++j) {
            if (j == self) continue;
            const V3<R> rij = pos1 - xyz<R>(sPos[j]);
            if (length(rij) < ir) {
                const R rhoNb = sDens[j];
                const R pNb = sPres[j];
                const V3<R> vel2 = xyz<R>(sVel[j]);
                const R diameter = (R)(2.0 * P.particleRadius);
                const R diameter2 = diameter * diameter;
                const V3<R> vij = vel1 - vel2;
                const R rhoSqOwn = dens * dens;
                const R rhoSqNb = rhoNb * rhoNb;
                V3<R> gradSpiky, gradVisc;
                R kernel, wAtDiameter;
                if (KSET == KS_MONAGHAN) {
                    gradSpiky = Wmonaghan_grad<R>(rij, ir);
                    gradVisc = gradSpiky;
                    kernel = Wmonaghan<R>(rij, ir);
                    wAtDiameter = Wmonaghan<R>(mk3<R>(diameter, 0, 0), ir);
                } else {
                    gradSpiky = Wpressure_grad<R>(rij, ir, kprg);
                    gradVisc = Wviscosity_grad<R>(rij, ir, kvg, kvd);
                    kernel = Wdefault<R>(rij, ir, kp);
                    wAtDiameter = Wdefault<R>(mk3<R>(diameter, 0, 0), ir, kp);
                }
                A.fpres = A.fpres + (m2 * (pres / rhoSqOwn + pNb / rhoSqNb) * gradSpiky);
                const R a = dot(rij, gradVisc);
                const R b = dot(rij, rij) + 0.01f * (ir * ir);
                A.fvisc = A.fvisc + (m2 / rhoNb * vij * (a / b));
                if (SURF) {
                    V3<R> ai = mk3<R>(0, 0, 0);
                    const R r2 = dot(rij, rij);
                    if (r2 > diameter2) ai = ai - (kappa / pm * pm * rij * kernel);
                    else ai = ai - (kappa / pm * pm * rij * wAtDiameter);
                    A.fsurf = A.fsurf + ai;
                }
            }
        }
    }
    if (HAS_B) {
        s = G.bCellStart[h];
        const R epsilon = (R)0.01;
        const R beta = P.beta;
        const R rd = P.restDensity;
        if (s != CELL_EMPTY) {
            const uint32_t e = G.bCellEnd[h];
            for (uint32_t j = s; j < e; ++j) { // no distance test on boundary particles (as the reference)
                const typename Vec4T<R>::type bq = G.sB[j];
                const R vbi = bq.w;
                const V3<R> vpos = xyz<R>(bq);
                const R psi = (rd * vbi);
                const V3<R> rij = pos1 - vpos;
                const V3<R> vij = vel1;
                R kernel;
                V3<R> grad;
                if (KSET == KS_MONAGHAN) {
                    kernel = Wmonaghan<R>(rij, ir);
                    grad = Wmonaghan_grad<R>(rij, ir);
                } else {
                    kernel = Wdefault<R>(rij, ir, P.kpoly);
                    grad = Wdefault_grad<R>(rij, ir, P.kpoly_grad);
                }
                A.fbound = A.fbound + (beta * psi * rij * kernel);
                A.fpres = A.fpres + (-pm * psi * (pres / (dens * dens)) * grad);
                const R nuWall = (P.viscosity * ir * P.soundSpeed) / (dens * dens);
                const R approach = (R)fmax((double)dot(vij, rij), 0.0);
                const R normSq = dot(rij / length(rij), rij / length(rij)) + epsilon * ir * ir;
                const R friction = -nuWall * (approach / normSq);
                A.fvisc = A.fvisc - (pm * psi * friction * grad);
            }
        }
    }
}

template <typename R, int KSET, bool SURF, bool HAS_B>
NRS_DEV ForceAcc<R> gather_forces(const Params<R> &P, const GridView<R> &G, uint32_t self, V3<R> pos, V3<R> vel, R dens,
                                  R pres, const typename Vec4T<R>::type *__restrict__ sPos,
                                  const typename Vec4T<R>::type *__restrict__ sVel, const R *__restrict__ sDens,
                                  const R *__restrict__ sPres)
{
    ForceAcc<R> A;
    A.fpres = A.fvisc = A.fsurf = A.fbound = mk3<R>(0, 0, 0);
    const I3 gp = calcGridPos<R>(P, pos);
    for (int z = -1; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int x = -1; x <= 1; x++) {
                const uint32_t h = calcGridHash<R>(P, gp.x + x, gp.y + y, gp.z + z);
                cell_forces<R, KSET, SURF, HAS_B>(P, G, A, h, self, pos, vel, dens, pres, sPos, sVel, sDens, sPres);
            }
    return A;
}

// final combination of computeForces (sph_kernel_impl.cuh:663-674)
template <typename R> NRS_DEV V3<R> sesph_total_force(const Params<R> &P, ForceAcc<R> A, R dens)
{
    const R m1 = P.particleMass;
    V3<R> fpres = A.fpres * dens;
    V3<R> fvisc = A.fvisc * 2.0;
    fpres = fpres * -(m1 / dens);
    fvisc = fvisc * (m1 * P.viscosity);
    const V3<R> grav = mk3<R>(P.gravity[0], P.gravity[1], P.gravity[2]);
    return fpres + fvisc + (grav * m1) + A.fsurf + A.fbound;
}

// ---- computeForces (sph_kernel_impl.cuh:609-680) -----------------------------------------------------
template <typename R, int KSET, bool SURF, bool HAS_B>
__global__ __launch_bounds__(BLOCK) void k_forces_ref(Params<R> P, GridView<R> G,
                                                      const typename Vec4T<R>::type *__restrict__ sPos,
                                                      const typename Vec4T<R>::type *__restrict__ sVel,
                                                      const R *__restrict__ sDens, const R *__restrict__ sPres,
                                                      typename Vec4T<R>::type *__restrict__ forces, uint32_t n)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const V3<R> pos = xyz<R>(sPos[i]);
    if (!slab_active<R>(P, G, pos.x)) { forces[i] = mk4<R>((R)0, (R)0, (R)0, (R)0); return; }
    const V3<R> vel = xyz<R>(sVel[i]);
    const R dens = sDens[i], pres = sPres[i];
    ForceAcc<R> A = gather_forces<R, KSET, SURF, HAS_B>(P, G, i, pos, vel, dens, pres, sPos, sVel, sDens, sPres);
    const V3<R> f = sesph_total_force<R>(P, A, dens);
    forces[i] = mk4<R>(f, (R)0);
}

// IISPH slab runs: the warm-start pressure of a particle (p0 = 0.5 p of the last step, sph_kernel_impl.cuh:1187) has to travel
// with it through the partition and the messages.  vel.w is free for that — iisph_integrate zeroes it every step
// (sph_kernel_impl.cuh:1654) — so the pressure rides there from nrs_slab_pack to nrs_slab_unpack.
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_pressure_to_velw(typename Vec4T<R>::type *__restrict__ vel, const R *__restrict__ pres, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) vel[i].w = pres[i];
}
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_velw_to_pressure(typename Vec4T<R>::type *__restrict__ vel, R *__restrict__ pres, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) { pres[i] = vel[i].w; vel[i].w = (R)0; }
}

// ---- integrate_functor (sph_kernel_impl.cuh:71-100): symplectic Euler, w components kept --------------
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_integrate(Params<R> P, typename Vec4T<R>::type *__restrict__ pos,
                                                     typename Vec4T<R>::type *__restrict__ vel,
                                                     const typename Vec4T<R>::type *__restrict__ forces, uint32_t n)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const R dt = P.timestep, m1 = P.particleMass;
    typename Vec4T<R>::type p4 = pos[i], v4 = vel[i];
    V3<R> p = xyz<R>(p4), v = xyz<R>(v4), frc = xyz<R>(forces[i]);
    const V3<R> accel = dt * frc / m1;
    v = v + accel;
    p = p + dt * v;
    pos[i] = mk4<R>(p, p4.w);
    vel[i] = mk4<R>(v, v4.w);
}

// =========================================== IISPH ====================================================
template <typename R> struct IisphArrays {
    typedef typename Vec4T<R>::type T4;
    R *densAdv, *densCorr, *P_l, *P_l_next, *aii;
    T4 *velAdv, *forcesAdv, *forcesP, *diiF, *diiB, *sumDij;
    T4 *diiSum; // diiF + diiB, formed once per step by the list-driven displacement kernel (the pressure kernel's neighbour
                // term reads only the sum: one 16-byte gather per neighbour and iteration instead of two)
    const uint32_t *inv; // inv[slot] = id of the reference thread that handles the slot
    // Set by the list-driven kernels when a value that NEIGHBOURS will gather (velAdv, dii, sumDij, P_l) is not finite or so large
    // that a product or difference of two such values could overflow.  The list walks visit only neighbours inside the kernel
    // support; the reference's 27-cell walks also multiply the zero gradient of a particle beyond it with expressions of those
    // values (0 * inf = NaN): identical only while everything stays finite.  The context then repeats the step with the
    // reference-order kernels (PressureSolvers::iisph_tail, nrs_solvers.h).  null: not watched.
    uint32_t *nonFinite;
};
// (1e12: the cube of it is still a finite float — fp64 builds pass scalars through float as well, SURVEY Q11 —; a fluid step has no
// quantity anywhere near it)
template <typename R> NRS_DEV R watch_limit() { return (R)1e12; }
template <typename R> NRS_DEV void watch_finite(uint32_t *flag, V3<R> v)
{
    const R lim = watch_limit<R>();
    if (flag && !((fabs(v.x) < lim) & (fabs(v.y) < lim) & (fabs(v.z) < lim))) *flag = 1u; // (false for NaN too)
}
template <typename R> NRS_DEV void watch_finite(uint32_t *flag, R v)
{
    if (flag && !(fabs(v) < watch_limit<R>())) *flag = 1u;
}
// sPres[i] = pres[index[i]]: the sorted warm-start pressures once more (a step repeated in reference order)
template <typename R>
static __global__ __launch_bounds__(BLOCK) void k_gather_scalar(const R *__restrict__ src, const uint32_t *__restrict__ index, R *__restrict__ dst, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) dst[i] = src[index[i]];
}

// computeIisphDensity (:770-846) is k_density_ref with pres == nullptr.

// The per-particle walks of the IISPH loops below are shared with the list-driven kernels (nrs_kernels_iisph.h), which take them
// for a particle whose hit list overflowed: one statement of each reference loop for both kernel paths.

// the dii sums of computeDisplacementFactor (sph_kernel_impl.cuh:851-963) + its two cell helpers (:689-765): df over the fluid,
// db over the boundary particles, one partial per cell; both added to the caller's values
template <typename R, int KSET, bool HAS_B>
NRS_DEV void displacement_walk(const Params<R> &P, const GridView<R> &G, const typename Vec4T<R>::type *__restrict__ sPos,
                               uint32_t i, V3<R> pos1, R dens, V3<R> &df, V3<R> &db)
{
    const R kpg = P.kpoly_grad, pm = P.particleMass, ir = P.interactionRadius, rd = P.restDensity;
    const I3 gp = calcGridPos<R>(P, pos1);
    for (int z = -1; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int x = -1; x <= 1; x++) {
                const uint32_t h = calcGridHash<R>(P, gp.x + x, gp.y + y, gp.z + z);
                V3<R> res = mk3<R>(0, 0, 0);
                const uint32_t s = G.cellStart[h];
                if (s != CELL_EMPTY) {
                    const uint32_t e = G.cellEnd[h];
                    for (uint32_t j = s; j < e; ++j) {
                        if (j == i) continue;
                        const V3<R> d = pos1 - xyz<R>(sPos[j]);
                        if (length(d) < ir) res = res - ((pm / (dens * dens)) * W_grad<R, KSET>(d, ir, kpg));
                    }
                }
                df = df + res;
                if (HAS_B) {
                    V3<R> rb = mk3<R>(0, 0, 0);
                    const uint32_t sb = G.bCellStart[h];
                    if (sb != CELL_EMPTY) {
                        const uint32_t e = G.bCellEnd[h];
                        for (uint32_t j = sb; j < e; ++j) {
                            const typename Vec4T<R>::type b = G.sB[j];
                            const V3<R> d = pos1 - xyz<R>(b);
                            if (length(d) < ir) rb = rb - (((rd * b.w) / (dens * dens)) * W_grad<R, KSET>(d, ir, kpg));
                        }
                    }
                    db = db + rb;
                }
            }
}

// the two sums of computeAdvectionFactor (sph_kernel_impl.cuh:1114-1218) + helpers (:968-1108): rho_adv (fluid partials to
// rho_advf, boundary partials to rho_advb) and a_ii, one partial per cell; all three added to the caller's values
template <typename R, int KSET, bool HAS_B>
NRS_DEV void advection_walk(const Params<R> &P, const GridView<R> &G, const IisphArrays<R> &I,
                            const typename Vec4T<R>::type *__restrict__ sPos, uint32_t i, V3<R> pos1, V3<R> vel1, V3<R> velAdv1,
                            R dens, V3<R> diif, V3<R> diib, R &rho_advf, R &rho_advb, R &aii)
{
    const R kpg = P.kpoly_grad, pm = P.particleMass, ir = P.interactionRadius, rd = P.restDensity, dt = P.timestep;
    const I3 gp = calcGridPos<R>(P, pos1);
    for (int z = -1; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int x = -1; x <= 1; x++) {
                const uint32_t h = calcGridHash<R>(P, gp.x + x, gp.y + y, gp.z + z);
                R res = (R)0.0;
                const uint32_t s = G.cellStart[h];
                if (s != CELL_EMPTY) {
                    const uint32_t e = G.cellEnd[h];
                    for (uint32_t j = s; j < e; ++j) {
                        if (j == i) continue;
                        const V3<R> vij = velAdv1 - xyz<R>(I.velAdv[j]);
                        const V3<R> d = pos1 - xyz<R>(sPos[j]);
                        if (length(d) < ir) res += (dt * pm * dot(vij, W_grad<R, KSET>(d, ir, kpg)));
                    }
                }
                rho_advf += res;
                if (HAS_B) {
                    R rb = (R)0.0;
                    const uint32_t sb = G.bCellStart[h];
                    if (sb != CELL_EMPTY) {
                        const uint32_t e = G.bCellEnd[h];
                        for (uint32_t j = sb; j < e; ++j) { // no cut-off: relies on W_grad == 0 beyond h (Q8)
                            const typename Vec4T<R>::type b = G.sB[j];
                            const V3<R> d = pos1 - xyz<R>(b);
                            rb += (dt * (rd * b.w) * dot(vel1, W_grad<R, KSET>(d, ir, kpg)));
                        }
                    }
                    rho_advb += rb;
                }
            }
    for (int z = -1; z <= 1; z++) // (no cut-off on either loop of a_ii: Q8)
        for (int y = -1; y <= 1; y++)
            for (int x = -1; x <= 1; x++) {
                const uint32_t h = calcGridHash<R>(P, gp.x + x, gp.y + y, gp.z + z);
                R res = (R)0.0;
                const uint32_t s = G.cellStart[h];
                if (s != CELL_EMPTY) {
                    const uint32_t e = G.cellEnd[h];
                    for (uint32_t j = s; j < e; ++j) {
                        if (j == i) continue;
                        const V3<R> d = pos1 - xyz<R>(sPos[j]);
                        const R dpi = (pm) / (dens * dens);
                        const V3<R> grad = W_grad<R, KSET>(d, ir, kpg);
                        const V3<R> dji = dpi * grad;
                        res += (pm * dot((diif + diib) - dji, grad));
                    }
                }
                aii += res;
                if (HAS_B) {
                    R rb = (R)0.0;
                    const uint32_t sb = G.bCellStart[h];
                    if (sb != CELL_EMPTY) {
                        const uint32_t e = G.bCellEnd[h];
                        for (uint32_t j = sb; j < e; ++j) {
                            const typename Vec4T<R>::type b = G.sB[j];
                            const V3<R> d = pos1 - xyz<R>(b);
                            const R psi = rd * b.w;
                            const R dpi = (pm) / (dens * dens);
                            const V3<R> grad = W_grad<R, KSET>(d, ir, kpg);
                            const V3<R> dji = dpi * grad;
                            rb += psi * dot((diif + diib) - dji, grad);
                        }
                    }
                    aii += rb;
                }
            }
}

// computeSumDijPj (sph_kernel_impl.cuh:1259-1325) + dijpjcell (:1224-1253): fluid neighbours only, one partial per cell;
// added to the caller's dijpj
template <typename R, int KSET>
NRS_DEV void sumdij_walk(const Params<R> &P, const GridView<R> &G, const IisphArrays<R> &I,
                         const typename Vec4T<R>::type *__restrict__ sPos, const R *__restrict__ sDens, uint32_t i, V3<R> pos1,
                         V3<R> &dijpj)
{
    const R ir = P.interactionRadius, pm = P.particleMass, kpg = P.kpoly_grad;
    const I3 gp = calcGridPos<R>(P, pos1);
    for (int z = -1; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int x = -1; x <= 1; x++) {
                const uint32_t h = calcGridHash<R>(P, gp.x + x, gp.y + y, gp.z + z);
                V3<R> res = mk3<R>(0, 0, 0);
                const uint32_t s = G.cellStart[h];
                if (s != CELL_EMPTY) {
                    const uint32_t e = G.cellEnd[h];
                    for (uint32_t j = s; j < e; ++j) {
                        if (j == i) continue;
                        const V3<R> d = pos1 - xyz<R>(sPos[j]);
                        const R densj = sDens[j];
                        res = res - ((pm / (densj * densj)) * I.P_l[j] * W_grad<R, KSET>(d, ir, kpg));
                    }
                }
                dijpj = dijpj + res;
            }
}

// NRS_FLAG_IISPH_SELF_BY_SLOT: inv[slot] = slot, so that the two kernels below skip the particle itself (SURVEY Q5 off)
static __global__ __launch_bounds__(BLOCK) void k_identity(uint32_t *__restrict__ a, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) a[i] = i;
}

// the boundary loops of computePressure / computePressureForce run j from the FLUID cell start to the BOUNDARY cell end,
// over the boundary array, in every cell that holds boundary particles.  f(b) for each such b (xyz + Vbi in w).
template <typename R, typename F> NRS_DEV void for_each_boundary_q6(const GridView<R> &G, uint32_t h, F &&f)
{
    if (G.bCellStart[h] != CELL_EMPTY) {
        const uint32_t s = G.cellStart[h], eB = G.bCellEnd[h];
        for (uint32_t j = s; j < eB; ++j) f(G.sB[j]);
    }
}

// the neighbour sums of computePressure (sph_kernel_impl.cuh:1330-1492), one accumulator each, no per-cell partials:
// FLUID: fsum over the fluid slots but `skip` (Q5: the callers pass inv[i], the reference thread id); dii(j) = diiF[j] + diiB[j]
// BOUND: bsum over the boundary particles of the Q6 range
template <typename R, int KSET, bool FLUID, bool BOUND, typename Dii>
NRS_DEV void pressure_walk(const Params<R> &P, const GridView<R> &G, const IisphArrays<R> &I,
                           const typename Vec4T<R>::type *__restrict__ sPos, uint32_t skip, V3<R> pos1, R dens, V3<R> dijpj,
                           Dii &&dii, R &fsum, R &bsum)
{
    const R ir = P.interactionRadius, pm = P.particleMass, kpg = P.kpoly_grad, rd = P.restDensity;
    const R dpi = pm / (dens * dens);
    auto term = [&](uint32_t j) {
        const V3<R> d = pos1 - xyz<R>(sPos[j]);
        const R p_lj = I.P_l[j];
        const V3<R> grad = W_grad<R, KSET>(d, ir, kpg);
        const V3<R> dji = dpi * (grad);
        const V3<R> d_ji_pi = dji * p_lj;
        const V3<R> diij = dii(j);
        const V3<R> sum_dijj = xyz<R>(I.sumDij[j]);
        fsum += pm * dot(dijpj - diij * p_lj - (sum_dijj - d_ji_pi), grad);
    };
    const I3 gp = calcGridPos<R>(P, pos1);
    for (int z = -1; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int x = -1; x <= 1; x++) {
                const uint32_t h = calcGridHash<R>(P, gp.x + x, gp.y + y, gp.z + z);
                if (FLUID) {
                    const uint32_t s = G.cellStart[h];
                    if (s != CELL_EMPTY) {
                        const uint32_t e = G.cellEnd[h];
                        for (uint32_t j = s; j < e; ++j)
                            if (j != skip) term(j);
                    }
                }
                if (BOUND)
                    for_each_boundary_q6<R>(G, h, [&](const typename Vec4T<R>::type &b) {
                        const V3<R> d = pos1 - xyz<R>(b);
                        const R psi = rd * b.w;
                        bsum += psi * dot(dijpj, W_grad<R, KSET>(d, ir, kpg));
                    });
            }
}

// the pressure force of computePressureForce (sph_kernel_impl.cuh:1497-1620): one accumulator takes the fluid terms of a cell and
// then that cell's boundary terms (Q6 range), cell by cell (c = 0..26, z, y, x).  fluidCell(c, h, term) calls term(j) for the cell's
// fluid slots but the reference thread id (Q5), ascending.
template <typename R, int KSET, bool HAS_B, typename FluidCell>
NRS_DEV V3<R> pforce_walk(const Params<R> &P, const GridView<R> &G, const typename Vec4T<R>::type *__restrict__ sPos,
                          const R *__restrict__ sDens, const R *__restrict__ sPres, V3<R> pos1, R p, R dens, FluidCell &&fluidCell)
{
    const R ir = P.interactionRadius, pm = P.particleMass, kpg = P.kpoly_grad, rd = P.restDensity;
    V3<R> fp = mk3<R>(0, 0, 0);
    auto term = [&](uint32_t j) {
        const V3<R> d = pos1 - xyz<R>(sPos[j]);
        const R pj = sPres[j];
        const R densj = sDens[j];
        const V3<R> grad = W_grad<R, KSET>(d, ir, kpg);
        const V3<R> contrib = -pm * pm * (p / (dens * dens) + pj / (densj * densj)) * grad;
        fp = fp + contrib;
    };
    const I3 gp = calcGridPos<R>(P, pos1);
    for (int c = 0; c < 27; ++c) {
        const int z = c / 9 - 1, y = (c / 3) % 3 - 1, x = c % 3 - 1;
        const uint32_t h = calcGridHash<R>(P, gp.x + x, gp.y + y, gp.z + z);
        fluidCell(c, h, term);
        if (HAS_B)
            for_each_boundary_q6<R>(G, h, [&](const typename Vec4T<R>::type &b) {
                const V3<R> d = pos1 - xyz<R>(b);
                const R psi = rd * b.w;
                const V3<R> contrib = (pm * psi * (p / (dens * dens)) * W_grad<R, KSET>(d, ir, kpg));
                fp = fp + contrib;
            });
    }
    return fp;
}
// the fluid cell walk of both computePressureForce paths: term(j) for the slots of cell h but skip
template <typename R, typename F> NRS_DEV void pforce_fluid_cell(const GridView<R> &G, uint32_t h, uint32_t skip, F &term)
{
    const uint32_t s = G.cellStart[h];
    if (s != CELL_EMPTY) {
        const uint32_t e = G.cellEnd[h];
        for (uint32_t j = s; j < e; ++j)
            if (j != skip) term(j);
    }
}

// computePressure (sph_kernel_impl.cuh:1330-1492): relaxed Jacobi, omega = 0.5.
// Q7: reads P_l, writes P_l_next (true Jacobi; the reference updates in place and races).
template <typename R, int KSET, bool HAS_B>
__global__ __launch_bounds__(BLOCK) void k_pressure_ref(Params<R> P, GridView<R> G, IisphArrays<R> I,
                                                        const typename Vec4T<R>::type *__restrict__ sPos,
                                                        const R *__restrict__ sDens, R *__restrict__ sPres, uint32_t n)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t skip = I.inv[i];
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const R dens = sDens[i];
    R p_l = I.P_l[i];
    const R previous_p_l = p_l;
    const R rho_adv = I.densAdv[i];
    const R aii = I.aii[i];
    const V3<R> dijpj = xyz<R>(I.sumDij[i]);
    const R dt = P.timestep, rd = P.restDensity;
    R fsum = (R)0.0, bsum = (R)0.0;
    pressure_walk<R, KSET, true, HAS_B>(P, G, I, sPos, skip, pos1, dens, dijpj,
                                        [&](uint32_t j) { return xyz<R>(I.diiF[j]) + xyz<R>(I.diiB[j]); }, fsum, bsum);
    const R omega = (R)0.5;
    R rho_corr = rho_adv + fsum + bsum;
    const R dt2 = dt * dt;
    const R diagDt2 = aii * dt2;
    const R b = rd - rho_adv;
    if (fabs(diagDt2) > 1.1920928955078125e-07f /* FLT_EPSILON */)
        p_l = (R)((1.0 - omega) * previous_p_l + (omega / diagDt2) * (b - dt2 * (bsum + fsum)));
    else
        p_l = (R)0.0;
    const R p = (R)fmax((double)p_l, 0.0);
    p_l = p;
    rho_corr += aii * previous_p_l;
    I.P_l_next[i] = p_l;
    sPres[i] = p_l;
    I.densCorr[i] = rho_corr;
}

// computeDisplacementFactor (sph_kernel_impl.cuh:851-963)
template <typename R, int KSET, bool SURF, bool HAS_B>
__global__ __launch_bounds__(BLOCK) void k_displacement_ref(Params<R> P, GridView<R> G, IisphArrays<R> I,
                                                            const typename Vec4T<R>::type *__restrict__ sPos,
                                                            const typename Vec4T<R>::type *__restrict__ sVel,
                                                            const R *__restrict__ sDens, const R *__restrict__ sPres,
                                                            uint32_t n)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const V3<R> vel1 = xyz<R>(sVel[i]);
    const R pres = (R)0.0;
    const R dens = sDens[i];
    const R pm = P.particleMass, dt = P.timestep;
    ForceAcc<R> A = gather_forces<R, KSET, SURF, HAS_B>(P, G, i, pos1, vel1, dens, pres, sPos, sVel, sDens, sPres);
    V3<R> fvisc = 2.0 * A.fvisc;
    fvisc = (pm * P.viscosity) * fvisc;
    const V3<R> fgrav = pm * mk3<R>(P.gravity[0], P.gravity[1], P.gravity[2]);
    const V3<R> force_adv = fvisc + A.fsurf + A.fbound + fgrav;
    const V3<R> vel_adv = vel1 + dt * (force_adv / pm);
    I.forcesAdv[i] = mk4<R>(force_adv, (R)0.0);
    I.velAdv[i] = mk4<R>(vel_adv, (R)0.0);
    V3<R> df = mk3<R>(0, 0, 0), db = mk3<R>(0, 0, 0);
    displacement_walk<R, KSET, HAS_B>(P, G, sPos, i, pos1, dens, df, db);
    I.diiF[i] = mk4<R>(df, (R)0.0);
    I.diiB[i] = mk4<R>(db, (R)0.0);
}

// computeAdvectionFactor (sph_kernel_impl.cuh:1114-1218)
template <typename R, int KSET, bool HAS_B>
__global__ __launch_bounds__(BLOCK) void k_advection_ref(Params<R> P, GridView<R> G, IisphArrays<R> I,
                                                         const typename Vec4T<R>::type *__restrict__ sPos,
                                                         const typename Vec4T<R>::type *__restrict__ sVel,
                                                         const R *__restrict__ sDens, const R *__restrict__ sPres,
                                                         uint32_t n)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const R dens = sDens[i];
    R rho_advf = (R)0.0, rho_advb = (R)0.0, aii = (R)0.0;
    advection_walk<R, KSET, HAS_B>(P, G, I, sPos, i, xyz<R>(sPos[i]), xyz<R>(sVel[i]), xyz<R>(I.velAdv[i]), dens, xyz<R>(I.diiF[i]),
                                   xyz<R>(I.diiB[i]), rho_advf, rho_advb, aii);
    const R rho_adv = dens + (rho_advf + rho_advb);
    I.densAdv[i] = rho_adv;
    I.P_l[i] = (R)(0.5 * sPres[i]);
    I.aii[i] = aii;
}

// computeSumDijPj (sph_kernel_impl.cuh:1259-1325)
template <typename R, int KSET>
__global__ __launch_bounds__(BLOCK) void k_sumdij_ref(Params<R> P, GridView<R> G, IisphArrays<R> I,
                                                      const typename Vec4T<R>::type *__restrict__ sPos,
                                                      const R *__restrict__ sDens, uint32_t n)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    V3<R> dijpj = mk3<R>(0, 0, 0);
    sumdij_walk<R, KSET>(P, G, I, sPos, sDens, i, xyz<R>(sPos[i]), dijpj);
    I.sumDij[i] = mk4<R>(dijpj, (R)0.0);
}

// computePressureForce (sph_kernel_impl.cuh:1497-1620)
template <typename R, int KSET, bool HAS_B>
__global__ __launch_bounds__(BLOCK) void k_pforce_ref(Params<R> P, GridView<R> G, IisphArrays<R> I,
                                                      const typename Vec4T<R>::type *__restrict__ sPos,
                                                      const R *__restrict__ sDens, const R *__restrict__ sPres,
                                                      uint32_t n)
{
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t skip = I.inv[i];
    const V3<R> fp = pforce_walk<R, KSET, HAS_B>(P, G, sPos, sDens, sPres, xyz<R>(sPos[i]), sPres[i], sDens[i],
                                                 [&](int, uint32_t h, auto &term) { pforce_fluid_cell<R>(G, h, skip, term); });
    I.forcesP[i] = mk4<R>(fp, (R)0.0);
}

// iisph_integrate (sph_kernel_impl.cuh:1625-1655): sets pos.w = 1, vel.w = 0
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_iisph_integrate(Params<R> P, typename Vec4T<R>::type *__restrict__ pos,
                                                           typename Vec4T<R>::type *__restrict__ vel,
                                                           const typename Vec4T<R>::type *__restrict__ velAdv,
                                                           const typename Vec4T<R>::type *__restrict__ forcesP,
                                                           uint32_t n, uint32_t *__restrict__ nextHash,
                                                           uint32_t *__restrict__ nextIndex, const uint32_t *__restrict__ prevHash,
                                                           uint32_t *__restrict__ tileMovers, int keepHaloMark)
{
    // nextHash/nextIndex (both or neither): also emit the next step's sort keys (calcHashD of the new position);
    // prevHash/tileMovers (both or neither): count the slots whose key changes, for the coherent re-sort
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const R dt = P.timestep, pm = P.particleMass;
    const V3<R> pos1 = xyz<R>(pos[i]);
    const V3<R> velAdv1 = xyz<R>(velAdv[i]);
    const V3<R> fpres1 = xyz<R>(forcesP[i]);
    const V3<R> newVel = velAdv1 + (dt * fpres1 / pm);
    const V3<R> newPos = pos1 + (dt * newVel);
    // the reference sets w = 1 / 0 here (sph_kernel_impl.cuh:1653-1654); slab runs keep the w = 2 that marks a halo copy (not a
    // particle of this rank: it is dropped by the next partition)
    const R w0 = pos[i].w;
    pos[i] = mk4<R>(newPos, (keepHaloMark && w0 == (R)2.0) ? (R)2.0 : (R)1.0);
    vel[i] = mk4<R>(newVel, (R)0.0);
    if (nextHash) {
        const I3 g = calcGridPos<R>(P, newPos);
        const uint32_t h = calcGridHash<R>(P, g.x, g.y, g.z);
        nextHash[i] = h;
        nextIndex[i] = i;
        if (tileMovers && h != prevHash[i]) atomicAdd(&tileMovers[i / BLOCK], 1u);
    }
}

// =========================================== PCISPH ===================================================
// Predictive-corrective incompressible SPH (Solenthaler & Pajarola 2009).  The reference leaves its PCISPH solve an empty stub
// (sph_cuda.cu:944-952), so DESIGN.md "PCISPH" defines what is computed here.  Every neighbour sum of the loop runs over the pairs
// with length(x_i - x_j) < h at the step's START positions (the neighbourhood of the step's density scan) AND length(x*_i - x*_j) < h
// at the predicted ones; boundary particles are static (x*_b = x_b); the fluid sums skip j == i by sorted slot.  Sums are formed in
// the order of density_of: cells z, y, x of the start cell, in each a fluid partial (j ascending) and then a boundary partial, each
// added to the running total — which both walks of nrs_kernels_walk.h keep.
template <typename R> struct PciArrays {
    typedef typename Vec4T<R>::type T4;
    T4 *velAdv, *forcesAdv, *forcesP; // vel_adv, the non-pressure force, the pressure force Fp
    R *densPred, *pres, *err;         // rho*, p, e = max(rho* - rho0, 0) / rho0 (input of the exit test's max)
    const T4 *xsIn;                   // predicted positions the launch reads (its own and its neighbours')
    T4 *xsOut;                        // ... and where the pressure-force launch writes the next ones (double-buffered)
    R delta;                          // the pressure scale: p += delta (rho* - rho0)
};
// (a scalar times a vector in SReal: the vector operators of nrs_math.h take float scalars, SURVEY Q11, which the PCISPH loop's own
// coefficients need not inherit)
template <typename R> NRS_DEV V3<R> pci_scale(R s, V3<R> v) { return mk3<R>(s * v.x, s * v.y, s * v.z); }
// the coefficients of the pressure force: fluid -m^2 (p_i + p_j) / rho0^2, boundary -m psi_b p_i / rho0^2 (psi_b = rho0 V_b)
template <typename R> NRS_DEV R pci_fluid_coef(const Params<R> &P, R p, R pj)
{
    const R pm = P.particleMass, rd = P.restDensity;
    return -(pm * pm) * ((p + pj) / (rd * rd));
}
template <typename R> NRS_DEV R pci_boundary_coef(const Params<R> &P, R psi, R p)
{
    const R pm = P.particleMass, rd = P.restDensity;
    return -(pm * psi) * (p / (rd * rd));
}
// x* = x + dt (vel_adv + dt Fp / m): the expression of k_iisph_integrate, so that the positions the last iteration predicts are the
// positions the step integrates to
template <typename R> NRS_DEV V3<R> pci_predict(const Params<R> &P, V3<R> pos1, V3<R> velAdv1, V3<R> fp)
{
    const R dt = P.timestep, pm = P.particleMass;
    const V3<R> v = velAdv1 + (dt * fp / pm);
    return pos1 + (dt * v);
}
// rho* -> p (clamped at 0) and e_i; NaN densities give e = inf (the loop then runs to its cap and reports it)
template <typename R> NRS_DEV void pci_pressure_update(const Params<R> &P, const PciArrays<R> &A, uint32_t i, R rs)
{
    const R rd = P.restDensity;
    const R dr = rs - rd;
    const R pn = A.pres[i] + A.delta * dr;
    A.densPred[i] = rs;
    A.pres[i] = pn > (R)0 ? pn : (R)0;
    A.err[i] = dr <= (R)0 ? (R)0 : (dr == dr ? dr / rd : (R)INFINITY);
}
// vel_adv = v + dt force_adv / m with the non-pressure forces of the IISPH displacement stage (k_displacement_ref's force half,
// which is also what the reference's never-launched pciComputePosVelAdv computes)
template <typename R> NRS_DEV V3<R> pci_advect_force(const Params<R> &P, const ForceAcc<R> &A)
{
    const R pm = P.particleMass;
    V3<R> fvisc = 2.0 * A.fvisc;
    fvisc = (pm * P.viscosity) * fvisc;
    const V3<R> fgrav = pm * mk3<R>(P.gravity[0], P.gravity[1], P.gravity[2]);
    return fvisc + A.fsurf + A.fbound + fgrav;
}
template <typename R> NRS_DEV void pci_advect_store(const Params<R> &P, const PciArrays<R> &A, uint32_t i, V3<R> pos1, V3<R> vel1,
                                                    V3<R> force_adv)
{
    const R pm = P.particleMass, dt = P.timestep;
    const V3<R> vel_adv = vel1 + dt * (force_adv / pm);
    const V3<R> zero = mk3<R>(0, 0, 0);
    A.forcesAdv[i] = mk4<R>(force_adv, (R)0.0);
    A.velAdv[i] = mk4<R>(vel_adv, (R)0.0);
    A.forcesP[i] = mk4<R>(zero, (R)0.0);
    A.pres[i] = (R)0.0;
    A.xsOut[i] = mk4<R>(pci_predict<R>(P, pos1, vel_adv, zero), (R)1.0);
}

// (kept hand-written: in the shared form of nrs_kernels_walk.h the fp32 list kernel with boundary code and without wall workgroups needs
// more than 96 VGPRs and loses a wave, DESIGN.md "One neighbour walk")
// pressure force on particle i (iteration launch B), reference order
template <typename R, int KSET, bool HAS_B>
NRS_DEV V3<R> pci_pforce_walk(const Params<R> &P, const GridView<R> &G, const typename Vec4T<R>::type *__restrict__ sPos,
                              const typename Vec4T<R>::type *__restrict__ xs, const R *__restrict__ pres, uint32_t i, V3<R> pos1,
                              V3<R> xs1, R p)
{
    const R ir = P.interactionRadius, kpg = P.kpoly_grad, rd = P.restDensity;
    const I3 gp = calcGridPos<R>(P, pos1);
    V3<R> fp = mk3<R>(0, 0, 0);
    for (int z = -1; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int x = -1; x <= 1; x++) {
                const uint32_t h = calcGridHash<R>(P, gp.x + x, gp.y + y, gp.z + z);
                V3<R> c = mk3<R>(0, 0, 0);
                const uint32_t s = G.cellStart[h];
                if (s != CELL_EMPTY) {
                    const uint32_t e = G.cellEnd[h];
                    for (uint32_t j = s; j < e; ++j) {
                        if (j == i || !(length(pos1 - xyz<R>(sPos[j])) < ir)) continue;
                        const V3<R> d = xs1 - xyz<R>(xs[j]);
                        if (length(d) < ir) c = c + pci_scale<R>(pci_fluid_coef<R>(P, p, pres[j]), W_grad<R, KSET>(d, ir, kpg));
                    }
                }
                fp = fp + c;
                if (HAS_B) {
                    V3<R> cb = mk3<R>(0, 0, 0);
                    const uint32_t sb = G.bCellStart[h];
                    if (sb != CELL_EMPTY) {
                        const uint32_t e = G.bCellEnd[h];
                        for (uint32_t j = sb; j < e; ++j) {
                            const typename Vec4T<R>::type b = G.sB[j];
                            if (!(length(pos1 - xyz<R>(b)) < ir)) continue;
                            const V3<R> d = xs1 - xyz<R>(b);
                            if (length(d) < ir) cb = cb + pci_scale<R>(pci_boundary_coef<R>(P, rd * b.w, p), W_grad<R, KSET>(d, ir, kpg));
                        }
                    }
                    fp = fp + cb;
                }
            }
    return fp;
}

// PCISPH advection: non-pressure forces, vel_adv, x*0 = x + dt vel_adv, p = 0, Fp = 0
template <typename R, int KSET, bool SURF, bool HAS_B>
__global__ __launch_bounds__(BLOCK) void k_pci_advect_ref(Params<R> P, GridView<R> G, PciArrays<R> A,
                                                          const typename Vec4T<R>::type *__restrict__ sPos,
                                                          const typename Vec4T<R>::type *__restrict__ sVel,
                                                          const R *__restrict__ sDens, const R *__restrict__ sPres, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const V3<R> pos1 = xyz<R>(sPos[i]), vel1 = xyz<R>(sVel[i]);
    const ForceAcc<R> F = gather_forces<R, KSET, SURF, HAS_B>(P, G, i, pos1, vel1, sDens[i], (R)0.0, sPos, sVel, sDens, sPres);
    pci_advect_store<R>(P, A, i, pos1, vel1, pci_advect_force<R>(P, F));
}
// iteration launch B: pressure force and the next predicted positions
template <typename R, int KSET, bool HAS_B>
__global__ __launch_bounds__(BLOCK) void k_pci_pforce_ref(Params<R> P, GridView<R> G, PciArrays<R> A,
                                                          const typename Vec4T<R>::type *__restrict__ sPos, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const V3<R> pos1 = xyz<R>(sPos[i]);
    const V3<R> fp = pci_pforce_walk<R, KSET, HAS_B>(P, G, sPos, A.xsIn, A.pres, i, pos1, xyz<R>(A.xsIn[i]), A.pres[i]);
    A.forcesP[i] = mk4<R>(fp, (R)0.0);
    A.xsOut[i] = mk4<R>(pci_predict<R>(P, pos1, xyz<R>(A.velAdv[i]), fp), (R)1.0);
}
// the prototype sums of delta: out[0..2] = sum_k g_k, out[3] = sum_k g_k . g_k, out[4] = neighbours, over the lattice points k s,
// k in Z^3, 0 < |k s| < h, with g_k = W_grad(-k s) (in double, k_z, k_y, k_x ascending).  One thread.
template <typename R, int KSET>
__global__ __launch_bounds__(64) void k_pci_prototype(Params<R> P, R spacing, int kmax, double *__restrict__ out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const R ir = P.interactionRadius, kpg = P.kpoly_grad;
    double sx = 0.0, sy = 0.0, sz = 0.0, gg = 0.0, cnt = 0.0;
    for (int z = -kmax; z <= kmax; ++z)
        for (int y = -kmax; y <= kmax; ++y)
            for (int x = -kmax; x <= kmax; ++x) {
                if (x == 0 && y == 0 && z == 0) continue;
                const V3<R> d = mk3<R>(-(R)x * spacing, -(R)y * spacing, -(R)z * spacing);
                if (!(length(d) < ir)) continue;
                const V3<R> g = W_grad<R, KSET>(d, ir, kpg);
                sx += (double)g.x; sy += (double)g.y; sz += (double)g.z;
                gg += (double)g.x * (double)g.x + (double)g.y * (double)g.y + (double)g.z * (double)g.z;
                cnt += 1.0;
            }
    out[0] = sx; out[1] = sy; out[2] = sz; out[3] = gg; out[4] = cnt;
}

// =========================================== PBF ===================================================
// Position-based fluids (Macklin & Mueller 2013): a density constraint solved by Jacobi projection.  The reference names it among
// its future works only; DESIGN.md "PBF" defines what is computed here.  The neighbour rule and the order of every sum are those of
// the PCISPH loop above (start-position AND predicted-position cut-off, j != i by sorted slot, static boundary particles, one
// fluid partial and then one boundary partial per cell in the order of density_of), as both walks of nrs_kernels_walk.h form them (the
// passes: nrs_kernels_pbf.h).  The advection launch is PCISPH's (k_pci_advect_*).
template <typename R> struct PbfArrays {
    typedef typename Vec4T<R>::type T4;
    R *densPred, *lambda, *err; // rho*, lambda, e = max(rho* - rho0, 0) / rho0 (input of the exit test's max)
    T4 *dx;                     // the correction of the last position launch
    const T4 *xsIn;             // predicted positions the launch reads (its own and its neighbours')
    T4 *xsOut;                  // ... and where the position launch writes the corrected ones (double-buffered)
    R eps;                      // the constraint-force mixing term: relaxation * D_proto
};
// grad W_spiky: Wpressure_grad for the Muller set, W_grad for Monaghan (inside the loop's cut-off h).  Defined as 0 at zero separation,
// where Wpressure_grad divides by |r| = 0.
template <typename R, int KSET> NRS_DEV V3<R> pbf_grad(const Params<R> &P, V3<R> r)
{
    if (!(length(r) > 0.0f)) return mk3<R>(0, 0, 0);
    if constexpr (KSET == KS_MULLER) return Wpressure_grad<R>(r, P.interactionRadius, P.kpress_grad);
    else return W_grad<R, KSET>(r, P.interactionRadius, P.kpoly_grad);
}
template <typename R> NRS_DEV R pbf_dot(V3<R> a, V3<R> b) { return a.x * b.x + a.y * b.y + a.z * b.z; } // (in SReal, unlike dot())
// (x* - x) / dt, the velocity a predicted position implies
template <typename R> NRS_DEV V3<R> pbf_vel(const Params<R> &P, V3<R> xs, V3<R> x)
{
    const R dt = P.timestep;
    return mk3<R>((xs.x - x.x) / dt, (xs.y - x.y) / dt, (xs.z - x.z) / dt);
}
// the sums of launch A: rho*, sum g (fluid and boundary), sum |g|^2 (fluid)
template <typename R> struct PbfSums {
    R rho, gg;
    V3<R> g;
    NRS_DEV void add(const PbfSums &o) { rho += o.rho; g = g + o.g; gg += o.gg; }
};
template <typename R> NRS_DEV PbfSums<R> pbf_zero()
{
    PbfSums<R> s;
    s.rho = s.gg = (R)0.0;
    s.g = mk3<R>(0, 0, 0);
    return s;
}
// one fluid neighbour of launch A at predicted separation d (its start-position test already passed)
template <typename R, int KSET> NRS_DEV void pbf_lambda_fluid(const Params<R> &P, V3<R> d, PbfSums<R> &s)
{
    const R ir = P.interactionRadius, pm = P.particleMass, rd = P.restDensity;
    if (!(length(d) < ir)) return;
    s.rho += pm * W_dens<R, KSET>(d, ir, P.kpoly);
    const V3<R> g = pci_scale<R>(pm / rd, pbf_grad<R, KSET>(P, d));
    s.g = s.g + g;
    s.gg += pbf_dot<R>(g, g);
}
// one boundary neighbour of launch A: psi_b = rho0 V_b
template <typename R, int KSET> NRS_DEV void pbf_lambda_boundary(const Params<R> &P, V3<R> d, R psi, PbfSums<R> &s)
{
    const R ir = P.interactionRadius, rd = P.restDensity;
    if (!(length(d) < ir)) return;
    s.rho += psi * W_dens<R, KSET>(d, ir, P.kpoly);
    s.g = s.g + pci_scale<R>(psi / rd, pbf_grad<R, KSET>(P, d));
}
// rho*, C, D -> lambda and e; NaN densities give e = inf (the loop then runs to its cap and reports it)
template <typename R> NRS_DEV void pbf_lambda_store(const Params<R> &P, const PbfArrays<R> &A, uint32_t i, const PbfSums<R> &s)
{
    const R rd = P.restDensity;
    const R c = s.rho / rd - (R)1.0;
    const R C = c > (R)0 ? c : (R)0;
    const R D = pbf_dot<R>(s.g, s.g) + s.gg;
    const R dr = s.rho - rd;
    A.densPred[i] = s.rho;
    A.lambda[i] = -C / (D + A.eps);
    A.err[i] = dr <= (R)0 ? (R)0 : (dr == dr ? dr / rd : (R)INFINITY);
}
// the terms of launch B: (lambda_i + lambda_j) g_ij and lambda_i g_ib
template <typename R, int KSET> NRS_DEV V3<R> pbf_correct_fluid(const Params<R> &P, V3<R> d, R li, R lj)
{
    if (!(length(d) < P.interactionRadius)) return mk3<R>(0, 0, 0);
    return pci_scale<R>(li + lj, pci_scale<R>(P.particleMass / P.restDensity, pbf_grad<R, KSET>(P, d)));
}
// the tensile correction s_corr of launch B: s_ij = -k (W(x*_ij) / W_q)^4, W_q = W((dq h, 0, 0)).  Its instances are kernels of their
// own (PbfCorrectPass<R, KSET, true>, nrs_kernels_pbf.h).
template <typename R> struct PbfTensile {
    R k, wq;
};
template <typename R, int KSET> NRS_DEV V3<R> pbf_correct_fluid_s(const Params<R> &P, V3<R> d, R li, R lj, const PbfTensile<R> &T)
{
    const R ir = P.interactionRadius;
    if (!(length(d) < ir)) return mk3<R>(0, 0, 0);
    const R r = W_dens<R, KSET>(d, ir, P.kpoly) / T.wq;
    const R r2 = r * r;
    const R s = -T.k * (r2 * r2);
    return pci_scale<R>(li + lj + s, pci_scale<R>(P.particleMass / P.restDensity, pbf_grad<R, KSET>(P, d)));
}
template <typename R, int KSET> NRS_DEV V3<R> pbf_correct_boundary(const Params<R> &P, V3<R> d, R psi, R li)
{
    if (!(length(d) < P.interactionRadius)) return mk3<R>(0, 0, 0);
    return pci_scale<R>(li, pci_scale<R>(psi / P.restDensity, pbf_grad<R, KSET>(P, d)));
}
template <typename R> NRS_DEV void pbf_correct_store(const PbfArrays<R> &A, uint32_t i, V3<R> xs1, V3<R> dx)
{
    A.dx[i] = mk4<R>(dx, (R)0.0);
    A.xsOut[i] = mk4<R>(xs1 + dx, (R)1.0);
}
// the XSPH term of one fluid neighbour: (m / rho0) W(d) (v_j - v_i)
template <typename R, int KSET> NRS_DEV V3<R> pbf_xsph_fluid(const Params<R> &P, V3<R> d, V3<R> vj, V3<R> vi)
{
    const R ir = P.interactionRadius;
    if (!(length(d) < ir)) return mk3<R>(0, 0, 0);
    return pci_scale<R>((P.particleMass / P.restDensity) * W_dens<R, KSET>(d, ir, P.kpoly), vj - vi);
}

// PBF integration: v = (x* - x) / dt (or, after the XSPH launch, the velocity it left), x = x* with pos.w kept, vel.w = 0.  The sort
// keys of the next step and the movers of the coherent re-sort as k_iisph_integrate emits them.
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_pbf_integrate(Params<R> P, typename Vec4T<R>::type *__restrict__ pos,
                                                         typename Vec4T<R>::type *__restrict__ vel,
                                                         const typename Vec4T<R>::type *__restrict__ xs, int velGiven, uint32_t n,
                                                         uint32_t *__restrict__ nextHash, uint32_t *__restrict__ nextIndex,
                                                         const uint32_t *__restrict__ prevHash, uint32_t *__restrict__ tileMovers)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const typename Vec4T<R>::type p0 = pos[i];
    const V3<R> newPos = xyz<R>(xs[i]);
    if (!velGiven) vel[i] = mk4<R>(pbf_vel<R>(P, newPos, xyz<R>(p0)), (R)0.0);
    pos[i] = mk4<R>(newPos, p0.w);
    if (nextHash) {
        const I3 g = calcGridPos<R>(P, newPos);
        const uint32_t h = calcGridHash<R>(P, g.x, g.y, g.z);
        nextHash[i] = h;
        nextIndex[i] = i;
        if (tileMovers && h != prevHash[i]) atomicAdd(&tileMovers[i / BLOCK], 1u);
    }
}
// the prototype sums of D: out[0..2] = sum_k g_k, out[3] = sum_k g_k . g_k, out[4] = neighbours, over the lattice points k s, k in Z^3,
// 0 < |k s| < h, with g_k = (m / rho0) grad W_spiky(-k s) (in double, k_z, k_y, k_x ascending).  One thread.
template <typename R, int KSET>
__global__ __launch_bounds__(64) void k_pbf_prototype(Params<R> P, R spacing, int kmax, double *__restrict__ out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const R ir = P.interactionRadius;
    double sx = 0.0, sy = 0.0, sz = 0.0, gg = 0.0, cnt = 0.0;
    for (int z = -kmax; z <= kmax; ++z)
        for (int y = -kmax; y <= kmax; ++y)
            for (int x = -kmax; x <= kmax; ++x) {
                if (x == 0 && y == 0 && z == 0) continue;
                const V3<R> d = mk3<R>(-(R)x * spacing, -(R)y * spacing, -(R)z * spacing);
                if (!(length(d) < ir)) continue;
                const V3<R> g = pci_scale<R>(P.particleMass / P.restDensity, pbf_grad<R, KSET>(P, d));
                sx += (double)g.x; sy += (double)g.y; sz += (double)g.z;
                gg += (double)g.x * (double)g.x + (double)g.y * (double)g.y + (double)g.z * (double)g.z;
                cnt += 1.0;
            }
    out[0] = sx; out[1] = sy; out[2] = sz; out[3] = gg; out[4] = cnt;
}

// W_q = W((dq h, 0, 0)), the reference value of s_corr, with the solver's own W.  One thread.
template <typename R, int KSET>
__global__ __launch_bounds__(64) void k_pbf_wq(Params<R> P, R dq, double *__restrict__ out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    out[0] = (double)W_dens<R, KSET>(mk3<R>(dq * P.interactionRadius, 0, 0), P.interactionRadius, P.kpoly);
}

// ---- vorticity confinement (integration stage, eps_v > 0) ------------------------------------------------------------------------------
// u = (x* - x) / dt, the velocity before XSPH.  Two launches ahead of k_pbf_integrate, over fluid neighbours only, with the XSPH walk's
// neighbour rule:  omega_i = sum_j (m / rho0) (u_i - u_j) x grad W_spiky(x*_ij), stored as (omega, |omega|);  then
// eta_i = sum_j (m / rho0) (|omega_j| - |omega_i|) grad W_spiky(x*_ij), N_i = eta_i / |eta_i| (0 when |eta_i| <= PBF_VORT_CUT |omega_i| / h,
// where eta is roundoff of a locally uniform |omega| and has no direction) and vel_i = v_i + dt eps_v (N_i x omega_i), v_i the XSPH
// velocity if XSPH ran, else u_i.  |omega| and |eta| are SReal norms (pbf_norm), not the float length() of the cut-off tests.
constexpr double PBF_VORT_CUT = 1e-3;
template <typename R> NRS_DEV V3<R> pbf_cross(V3<R> a, V3<R> b)
{
    return mk3<R>(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
template <typename R> NRS_DEV R pbf_norm(V3<R> a) { return sqrt(pbf_dot<R>(a, a)); }
// one fluid neighbour of the vorticity sum: (m / rho0) (u_i - u_j) x grad W_spiky(d)
template <typename R, int KSET> NRS_DEV V3<R> pbf_vort_fluid(const Params<R> &P, V3<R> d, V3<R> uj, V3<R> ui)
{
    if (!(length(d) < P.interactionRadius)) return mk3<R>(0, 0, 0);
    return pbf_cross<R>(ui - uj, pci_scale<R>(P.particleMass / P.restDensity, pbf_grad<R, KSET>(P, d)));
}
// one fluid neighbour of the confinement sum: (m / rho0) (|omega_j| - |omega_i|) grad W_spiky(d)
template <typename R, int KSET> NRS_DEV V3<R> pbf_eta_fluid(const Params<R> &P, V3<R> d, R wj, R wi)
{
    if (!(length(d) < P.interactionRadius)) return mk3<R>(0, 0, 0);
    return pci_scale<R>((P.particleMass / P.restDensity) * (wj - wi), pbf_grad<R, KSET>(P, d));
}
template <typename R> NRS_DEV typename Vec4T<R>::type pbf_vort_pack(V3<R> w) { return mk4<R>(w, pbf_norm<R>(w)); }
// v + dt eps_v (N x omega)
template <typename R>
NRS_DEV V3<R> pbf_confine(const Params<R> &P, V3<R> v, V3<R> eta, typename Vec4T<R>::type om, R epsV)
{
    const R en = pbf_norm<R>(eta);
    if (!(en > (R)PBF_VORT_CUT * om.w / P.interactionRadius)) return v;
    const V3<R> N = pci_scale<R>((R)1.0 / en, eta);
    return v + pci_scale<R>(P.timestep * epsV, pbf_cross<R>(N, xyz<R>(om)));
}
// =========================================== DFSPH ===================================================
// Divergence-free SPH (Bender & Koschier 2015 / 2017): a divergence solve on the step's velocities and a density solve on vel_adv,
// both Jacobi iterations on velocities with PBF's spiky gradient.  DESIGN.md "DFSPH" defines what is computed here.  Every position is
// the step's START position (DFSPH moves no particle before the integration), so one neighbour rule holds for the whole step:
// length(x_i - x_j) < h, j != i by sorted slot, static boundary particles with the same rule.  Sums are formed in the order of
// density_of (one fluid partial and then one boundary partial per cell), as both walks of nrs_kernels_walk.h form them (the passes:
// nrs_kernels_dfsph.h).  g_ij = (m / rho0) pbf_grad(x_i - x_j), g_ib = (psi_b / rho0) pbf_grad(x_i - x_b).
template <typename R> struct DfsphArrays {
    typedef typename Vec4T<R>::type T4;
    T4 *u;         // the velocities the solve corrects, in place (the divergence solve: the sorted v; the density solve: vel_adv)
    const R *dens; // rho of the step's density scan
    R *alpha;      // 1 / D_i, or 0 where D_i <= thr (the factor launch)
    R *kappa;      // kappa_i of the last A launch (B reads its own and its neighbours')
    R *K;          // the running total K_i (m^2), in place: the sorted K_prev of the step when the solve starts
    R *err;        // e_i of the last A launch (input of the exit test's average)
    R *rhoAdv;     // density mode: rho_adv of the last A launch
    R thr;         // 1e-6 D_proto
};
// K's warm start: kappa_i = DFSPH_WARM K_prev_i / dt^2 where e_i > 0 (a constant, not a setting)
constexpr double DFSPH_WARM = 0.5;
// the A launch's phases: the warm-start A (kappa and K from K_prev), the first iteration (K = e alpha) and the later ones (K += e alpha)
enum { DFSPH_PHASE_WARM = 0, DFSPH_PHASE_FIRST = 1, DFSPH_PHASE_MORE = 2 };
template <typename R, int KSET> NRS_DEV V3<R> dfsph_g(const Params<R> &P, V3<R> d, R w)
{
    return pci_scale<R>(w / P.restDensity, pbf_grad<R, KSET>(P, d));
}
// the factor sums: sum g (fluid and boundary), sum |g|^2 (fluid)
template <typename R> struct DfsphFac {
    V3<R> g;
    R gg;
    NRS_DEV void add(const DfsphFac &o) { g = g + o.g; gg += o.gg; }
};
template <typename R> NRS_DEV DfsphFac<R> dfsph_fac_zero()
{
    DfsphFac<R> s;
    s.g = mk3<R>(0, 0, 0);
    s.gg = (R)0.0;
    return s;
}
// one fluid / boundary neighbour of the factor launch at separation d (its cut-off test already passed)
template <typename R, int KSET> NRS_DEV void dfsph_fac_fluid(const Params<R> &P, V3<R> d, DfsphFac<R> &s)
{
    const V3<R> g = dfsph_g<R, KSET>(P, d, P.particleMass);
    s.g = s.g + g;
    s.gg += pbf_dot<R>(g, g);
}
template <typename R, int KSET> NRS_DEV void dfsph_fac_boundary(const Params<R> &P, V3<R> d, R psi, DfsphFac<R> &s)
{
    s.g = s.g + dfsph_g<R, KSET>(P, d, psi);
}
template <typename R> NRS_DEV void dfsph_fac_store(const DfsphArrays<R> &A, uint32_t i, const DfsphFac<R> &s)
{
    const R D = pbf_dot<R>(s.g, s.g) + s.gg;
    A.alpha[i] = D > A.thr ? (R)1.0 / D : (R)0.0;
}
// the terms of launch A: (u_i - u_j) . g_ij and u_i . g_ib
template <typename R, int KSET> NRS_DEV R dfsph_div_fluid(const Params<R> &P, V3<R> d, V3<R> ui, V3<R> uj)
{
    return pbf_dot<R>(ui - uj, dfsph_g<R, KSET>(P, d, P.particleMass));
}
template <typename R, int KSET> NRS_DEV R dfsph_div_boundary(const Params<R> &P, V3<R> d, R psi, V3<R> ui)
{
    return pbf_dot<R>(ui, dfsph_g<R, KSET>(P, d, psi));
}
// div_i -> e_i, kappa_i, K_i (and rho_adv_i in density mode); NaN errors give e = inf (the loop then runs to its cap)
template <typename R, bool DENS> NRS_DEV void dfsph_div_store(const Params<R> &P, const DfsphArrays<R> &A, uint32_t i, R div, int phase)
{
    const R dt = P.timestep, rd = P.restDensity;
    R e;
    if constexpr (DENS) {
        const R ra = A.dens[i] + (dt * rd) * div;
        const R dr = ra - rd;
        A.rhoAdv[i] = ra;
        e = dr <= (R)0 ? (R)0 : (dr == dr ? dr / rd : (R)INFINITY);
    } else {
        const R x = dt * div;
        e = x <= (R)0 ? (R)0 : (x == x ? x : (R)INFINITY);
    }
    A.err[i] = e;
    const R dt2 = dt * dt;
    if (phase == DFSPH_PHASE_WARM) {
        const R kappa = e > (R)0 ? ((R)DFSPH_WARM * A.K[i]) / dt2 : (R)0.0;
        A.kappa[i] = kappa;
        A.K[i] = kappa * dt2;
    } else {
        const R ea = e * A.alpha[i];
        A.kappa[i] = ea / dt2;
        A.K[i] = (phase == DFSPH_PHASE_FIRST ? (R)0.0 : A.K[i]) + ea;
    }
}
// the terms of launch B: (kappa_i + kappa_j) g_ij and kappa_i g_ib
template <typename R, int KSET> NRS_DEV V3<R> dfsph_vup_fluid(const Params<R> &P, V3<R> d, R ki, R kj)
{
    return pci_scale<R>(ki + kj, dfsph_g<R, KSET>(P, d, P.particleMass));
}
template <typename R, int KSET> NRS_DEV V3<R> dfsph_vup_boundary(const Params<R> &P, V3<R> d, R psi, R ki)
{
    return pci_scale<R>(ki, dfsph_g<R, KSET>(P, d, psi));
}
// u_i -= dt sum (w kept)
template <typename R> NRS_DEV void dfsph_vup_store(const Params<R> &P, const DfsphArrays<R> &A, uint32_t i, typename Vec4T<R>::type u, V3<R> s)
{
    A.u[i] = mk4<R>(xyz<R>(u) - pci_scale<R>(P.timestep, s), u.w);
}

// (kept hand-written: in the shared form of nrs_kernels_walk.h the fp32 list kernel with boundary code and without wall workgroups needs
// more than 96 VGPRs and loses a wave, DESIGN.md "One neighbour walk")
// the velocity correction sum of particle i (launch B), reference order
template <typename R, int KSET, bool HAS_B>
NRS_DEV V3<R> dfsph_vup_walk(const Params<R> &P, const GridView<R> &G, const typename Vec4T<R>::type *__restrict__ sPos,
                             const R *__restrict__ kappa, uint32_t i, V3<R> pos1, R ki)
{
    const R ir = P.interactionRadius, rd = P.restDensity;
    const I3 gp = calcGridPos<R>(P, pos1);
    V3<R> sum = mk3<R>(0, 0, 0);
    for (int z = -1; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int x = -1; x <= 1; x++) {
                const uint32_t h = calcGridHash<R>(P, gp.x + x, gp.y + y, gp.z + z);
                V3<R> c = mk3<R>(0, 0, 0);
                const uint32_t s = G.cellStart[h];
                if (s != CELL_EMPTY) {
                    const uint32_t e = G.cellEnd[h];
                    for (uint32_t j = s; j < e; ++j) {
                        const V3<R> d = pos1 - xyz<R>(sPos[j]);
                        if (j == i || !(length(d) < ir)) continue;
                        c = c + dfsph_vup_fluid<R, KSET>(P, d, ki, kappa[j]);
                    }
                }
                sum = sum + c;
                if (HAS_B) {
                    V3<R> cb = mk3<R>(0, 0, 0);
                    const uint32_t sb = G.bCellStart[h];
                    if (sb != CELL_EMPTY) {
                        const uint32_t e = G.bCellEnd[h];
                        for (uint32_t j = sb; j < e; ++j) {
                            const typename Vec4T<R>::type b = G.sB[j];
                            const V3<R> d = pos1 - xyz<R>(b);
                            if (!(length(d) < ir)) continue;
                            cb = cb + dfsph_vup_boundary<R, KSET>(P, d, rd * b.w, ki);
                        }
                    }
                    sum = sum + cb;
                }
            }
    return sum;
}
// launch B: u_i -= dt (sum_j (kappa_i + kappa_j) g_ij + sum_b kappa_i g_ib), in place (B reads only its own u_i)
template <typename R, int KSET, bool HAS_B>
__global__ __launch_bounds__(BLOCK) void k_dfsph_vupdate_ref(Params<R> P, GridView<R> G, DfsphArrays<R> A,
                                                             const typename Vec4T<R>::type *__restrict__ sPos, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const typename Vec4T<R>::type u = A.u[i];
    dfsph_vup_store<R>(P, A, i, u, dfsph_vup_walk<R, KSET, HAS_B>(P, G, sPos, A.kappa, i, xyz<R>(sPos[i]), A.kappa[i]));
}

// deterministic two-pass sum of an SReal array in double (replaces thrust::reduce, sph_cuda.cu:816-819)
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_sum_partial(const R *__restrict__ a, double *__restrict__ partial, uint32_t n,
                                                       const typename Vec4T<R>::type *__restrict__ ownedPos = nullptr,
                                                       unsigned long long *__restrict__ ownedCount = nullptr)
{
    // ownedPos (slab runs): only the slots that hold a particle of this rank (pos.w == 1) count; their number goes to ownedCount
    __shared__ double sm[BLOCK / 64];
    double acc = 0.0;
    unsigned long long cnt = 0;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        if (ownedPos && !(ownedPos[i].w == (R)1.0)) continue;
        acc += (double)a[i];
        ++cnt;
    }
    if (ownedCount) {
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(ownedCount, cnt);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < BLOCK / 64; ++w) t += sm[w];
        partial[blockIdx.x] = t;
    }
}
static __global__ __launch_bounds__(BLOCK) void k_sum_final(const double *__restrict__ partial, double *__restrict__ out,
                                                     uint32_t nblocks)
{
    __shared__ double sm[BLOCK / 64];
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < nblocks; i += BLOCK) acc += partial[i];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < BLOCK / 64; ++w) t += sm[w];
        *out = t;
    }
}

// max of an SReal array / of |v| over a vec4 array (maxDensity / maxVelocity, sph_cuda.cu:32-53)
template <typename R, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_max_partial(const void *__restrict__ a, double *__restrict__ partial,
                                                       uint32_t n)
{
    __shared__ double sm[BLOCK / 64];
    double acc = -1.0e300;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        double v;
        if (VEC) {
            typename Vec4T<R>::type q = ((const typename Vec4T<R>::type *)a)[i];
            v = sqrt((double)q.x * q.x + (double)q.y * q.y + (double)q.z * q.z);
        } else {
            v = (double)((const R *)a)[i];
        }
        acc = fmax(acc, v);
    }
    for (int off = 32; off > 0; off >>= 1) acc = fmax(acc, __shfl_down(acc, off, 64));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sm[0];
        for (int w = 1; w < BLOCK / 64; ++w) t = fmax(t, sm[w]);
        partial[blockIdx.x] = t;
    }
}

} // namespace nrs
