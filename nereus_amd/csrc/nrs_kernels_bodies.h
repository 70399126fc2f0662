// nrs_kernels_bodies.h — kinematic boundary bodies (DESIGN.md "Kinematic boundary bodies").
//
// Boundary particles are grouped into rigid bodies (nrs_set_boundary_bodies); body 0 is the static world.  At the start of every step
// of a moving context the host advances the poses in double and hands the table below to the kernels here as a kernel argument, all
// of it rounded to SReal.  The boundary tables are then rebuilt on the device, on the context's stream, with no host wait:
//
//   k_boundary_pose_hash   world position of every boundary particle (upload order) + its (hash, index) pair, k_hash's arithmetic
//   rocPRIM radix sort     of the pairs, in storage the context owns
//   k_reorder_boundary_bodies   k_reorder_boundary + the sorted body id and the sorted wall velocity u_b
//   k_mark_near_boundary   (nrs_kernels_tiled.h) on the cleared near-boundary bits
//
// World position of a particle of body k >= 1 with rest position r (all SReal, no contraction, in exactly this order):
//   d   = r - c_k                                             (per component)
//   p_i = x_k[i] + ((R_k[i][0] d_0 + R_k[i][1] d_1) + R_k[i][2] d_2)
// Particles of body 0 are copied: their bits are those of the upload.  Wall velocity of a sorted boundary particle at p of body k:
//   a   = p - x_k
//   u_b = v_k + (w_y a_z - w_z a_y, w_z a_x - w_x a_z, w_x a_y - w_y a_x),      u_b = 0 for body 0.
//
// DFSPH is the one solver that works at the velocity level: its A launch uses sum_b (u_i - u_b) . g_ib while the context is moving
// (DfsphDivPass's MOVING flag and dfsph_div_boundary_mv, nrs_kernels_dfsph.h: the same walks as every other pass, so the two kernel
// paths give the same bits).  B is unchanged: the boundary carries no kappa.
#pragma once
#include "nrs_kernels_dfsph.h"

namespace nrs {

// one rigid body, as the kernels see it: rotation (row-major), origin now, origin at rest, linear and angular velocity
template <typename R> struct BodyPose { R rot[9]; R x[3]; R c[3]; R v[3]; R w[3]; };
template <typename R> struct BodyTable { BodyPose<R> b[NRS_MAX_BODIES]; }; // (entry 0, the static world, is never read)

template <typename R> NRS_DEV V3<R> body_transform(const BodyPose<R> &B, V3<R> r)
{
#pragma clang fp contract(off)
    const R d0 = r.x - B.c[0], d1 = r.y - B.c[1], d2 = r.z - B.c[2];
    const R px = B.x[0] + ((B.rot[0] * d0 + B.rot[1] * d1) + B.rot[2] * d2);
    const R py = B.x[1] + ((B.rot[3] * d0 + B.rot[4] * d1) + B.rot[5] * d2);
    const R pz = B.x[2] + ((B.rot[6] * d0 + B.rot[7] * d1) + B.rot[8] * d2);
    return mk3<R>(px, py, pz);
}
template <typename R> NRS_DEV V3<R> body_velocity(const BodyPose<R> &B, V3<R> p)
{
#pragma clang fp contract(off)
    const R ax = p.x - B.x[0], ay = p.y - B.x[1], az = p.z - B.x[2];
    const R ux = B.v[0] + (B.w[1] * az - B.w[2] * ay);
    const R uy = B.v[1] + (B.w[2] * ax - B.w[0] * az);
    const R uz = B.v[2] + (B.w[0] * ay - B.w[1] * ax);
    return mk3<R>(ux, uy, uz);
}

// one thread per boundary particle in upload order: world position (w = V_b) and the (hash, index) pair of k_hash
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_boundary_pose_hash(Params<R> P, BodyTable<R> T, const typename Vec4T<R>::type *__restrict__ rest,
                                                              const R *__restrict__ vbi, const uint32_t *__restrict__ bodyOf,
                                                              typename Vec4T<R>::type *__restrict__ world, uint32_t *__restrict__ hash,
                                                              uint32_t *__restrict__ index, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const typename Vec4T<R>::type r4 = rest[i];
    const uint32_t k = bodyOf[i];
    V3<R> p = xyz<R>(r4);
    if (k != 0u && k < (uint32_t)NRS_MAX_BODIES) p = body_transform<R>(T.b[k], p);
    world[i] = mk4<R>(p, vbi[i]);
    const I3 g = calcGridPos<R>(P, p);
    hash[i] = calcGridHash<R>(P, g.x, g.y, g.z);
    index[i] = i;
}

// k_reorder_boundary on the world positions, plus the sorted body id and the sorted wall velocity
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_reorder_boundary_bodies(const uint32_t *__restrict__ hash, const uint32_t *__restrict__ index,
                                                                   BodyTable<R> T, const typename Vec4T<R>::type *__restrict__ world,
                                                                   const uint32_t *__restrict__ bodyOf,
                                                                   typename Vec4T<R>::type *__restrict__ sB, uint32_t *__restrict__ sBody,
                                                                   typename Vec4T<R>::type *__restrict__ sVel,
                                                                   uint32_t *__restrict__ cellStart, uint32_t *__restrict__ cellEnd, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
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
    const typename Vec4T<R>::type b = world[src];
    const uint32_t k = bodyOf[src];
    sB[i] = b;
    sBody[i] = k;
    V3<R> u = mk3<R>(0, 0, 0);
    if (k != 0u && k < (uint32_t)NRS_MAX_BODIES) u = body_velocity<R>(T.b[k], xyz<R>(b));
    sVel[i] = mk4<R>(u, (R)0.0);
}

// the sorted body ids of a context that has bodies but has not moved yet: a gather through the sorted indices
static __global__ __launch_bounds__(BLOCK) void k_gather_body(const uint32_t *__restrict__ index, const uint32_t *__restrict__ bodyOf,
                                                              uint32_t *__restrict__ sBody, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) sBody[i] = bodyOf[index[i]];
}

} // namespace nrs
