// nrs_host_surface.h — the host decisions of the surface extraction (include/nereus_hip.h "surface extraction"; DESIGN.md "Surface
// extraction") and the rules of marching tetrahedra on the sampler's lattice, written once: which calls and lattices are accepted, how
// many bytes a result takes, which result of the last extract an id means; the Kuhn tetrahedra of a cell, the seven edges a node owns,
// the 16 cases of a tetrahedron; the per-node routine (edge mask and vertex count) and the per-cell routine (triangle count, and the
// (corner, edge number) pair of every triangle index).  No HIP: the kernels (nrs_kernels_surface.h) and a plain host program
// (tests/host_surface_main.cpp) call the same routines; NRS_SURF_HD is empty without hipcc.
#pragma once
#include "nrs_host_sample.h"

#if defined(__HIPCC__)
#define NRS_SURF_HD __host__ __device__ inline
#define NRS_SURF_UNROLL _Pragma("unroll")
#else
#define NRS_SURF_HD inline
#define NRS_SURF_UNROLL
#endif

namespace nrs {

constexpr uint32_t SURFACE_ATTRIBUTES = NRS_SURFACE_GRADIENT | NRS_SURFACE_VELOCITY;
constexpr uint32_t SURFACE_KNOWN = SURFACE_ATTRIBUTES | NRS_SURFACE_WALLS;
// 7 vertices and 12 triangles per node at the most: with 2^27 nodes every vertex number, offset and total fits 32 bits by construction
constexpr uint64_t SURFACE_MAX_NODES = 1ull << 27;

// ---- what a call may ask for -------------------------------------------------------------------------------------------------------
static inline int surface_check_call(double iso, uint32_t flags)
{
    if (!std::isfinite(iso) || !(iso > 0.0)) return fail(NRS_E_INVALID, "iso must be finite and > 0");
    if (flags & ~SURFACE_KNOWN) return fail(NRS_E_INVALID, "flags has unknown bits");
    return NRS_OK;
}
// the sampler's own lattice rules, then: cells need two nodes per axis, offsets need the node cap
static inline int surface_check_lattice(const nrs_lattice *L, uint64_t *nodes)
{
    uint64_t n = 0;
    NRSCHK(sample_check_lattice(L, &n));
    for (int a = 0; a < 3; ++a)
        if (L->dims[a] < 2u) return fail(NRS_E_INVALID, "surface extraction needs a lattice dim >= 2 on every axis (there are no cells otherwise)");
    if (n > SURFACE_MAX_NODES) return fail(NRS_E_INVALID, "surface extraction on a lattice of more than 2^27 nodes");
    if (nodes) *nodes = n;
    return NRS_OK;
}
// the NRS_FIELD_* flags of the sample call an extract starts with
static inline uint32_t surface_sample_fields(uint32_t flags)
{
    return NRS_FIELD_DENSITY | ((flags & NRS_SURFACE_GRADIENT) ? NRS_FIELD_GRADIENT : 0u) | ((flags & NRS_SURFACE_VELOCITY) ? NRS_FIELD_VELOCITY : 0u) |
           ((flags & NRS_SURFACE_WALLS) ? NRS_FIELD_WALLS : 0u);
}

// ---- bytes of a result: `which` is ONE NRS_MESH_* id, V / T the totals of the extract, precision 32 or 64; 0 for anything else -----------
static inline uint64_t surface_result_bytes(uint32_t which, uint64_t V, uint64_t T, int precision)
{
    const uint64_t vec4 = precision == 64 ? 32 : 16;
    switch (which) {
    case NRS_MESH_VERTICES: case NRS_MESH_GRADIENT: case NRS_MESH_VELOCITY: return vec4 * V;
    case NRS_MESH_TRIANGLES: return 12 * T;
    default: return 0;
    }
}

// ---- which result an id means: the last extract's, or a refusal ------------------------------------------------------------------------
struct SurfaceLast {
    bool any = false;   // an extract has completed since nrs_create / nrs_surface_release
    uint32_t flags = 0; // its flags
    uint64_t V = 0, T = 0;
};
static inline int surface_route_result(const SurfaceLast &last, uint32_t which, int precision, uint64_t *bytes)
{
    if (which != NRS_MESH_VERTICES && which != NRS_MESH_TRIANGLES && which != NRS_MESH_GRADIENT && which != NRS_MESH_VELOCITY)
        return fail(NRS_E_INVALID, "which must be one of NRS_MESH_VERTICES, _TRIANGLES, _GRADIENT, _VELOCITY");
    if (!last.any) return fail(NRS_E_STATE, "no surface extract yet (or nrs_surface_release since)");
    if (which == NRS_MESH_GRADIENT && !(last.flags & NRS_SURFACE_GRADIENT)) return fail(NRS_E_STATE, "the last surface extract did not compute the gradient attribute");
    if (which == NRS_MESH_VELOCITY && !(last.flags & NRS_SURFACE_VELOCITY)) return fail(NRS_E_STATE, "the last surface extract did not compute the velocity attribute");
    *bytes = surface_result_bytes(which, last.V, last.T, precision);
    return NRS_OK;
}

// ---- the lattice as the routines get it (Lattice, nrs_host_sample.h) ------------------------------------------------------------------------
// coordinate `a` of the node with index idx on that axis: (R)(origin + idx * spacing), product and sum in double, one rounding to R
// (the sampler's lattice_node)
template <typename R> NRS_SURF_HD R surf_node_coord(const Lattice &L, int a, uint32_t idx) { return (R)(L.origin[a] + (double)idx * L.spacing[a]); }
// which of the three + neighbours of node (i, j, k) exist: bit a set when idx[a] + 1 < dims[a]; 7: the node is the low corner of a cell
NRS_SURF_HD uint32_t surf_have(const Lattice &L, uint32_t i, uint32_t j, uint32_t k)
{
    return (i + 1u < L.dims[0] ? 1u : 0u) | (j + 1u < L.dims[1] ? 2u : 0u) | (k + 1u < L.dims[2] ? 4u : 0u);
}

// ---- corners, edges, tetrahedra ---------------------------------------------------------------------------------------------------------
// A corner of a cell, and the direction of an edge, is a 3-bit code dx | dy << 1 | dz << 2.  A node owns the seven edges towards +,
// numbered (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1): codes 1, 2, 4, 3, 5, 6, 7.
NRS_SURF_HD uint32_t surf_edge_dir(uint32_t e) { return (0x7653421u >> (4u * e)) & 7u; }  // edge number 0..6 -> direction code
NRS_SURF_HD uint32_t surf_dir_edge(uint32_t d) { return (0x65423100u >> (4u * d)) & 7u; } // direction code 1..7 -> edge number
// The six Kuhn tetrahedra of a cell, one per permutation (a, b, c) of the axes in lexicographic order xyz, xzy, yxz, yzx, zxy, zyx: corners
// 000, +e_a, +e_a+e_b, 111 (tet-local numbers 0..3).  All share the body diagonal; the face diagonals are the edges 3, 4, 5 of a node, so
// neighbouring cells agree on them.  Each corner's code contains the one before: the edge between local corners p < q belongs to the
// node of corner p and has the direction code(q) ^ code(p).
NRS_SURF_HD uint32_t surf_tet_axis_a(uint32_t t) { return t >> 1; }
NRS_SURF_HD uint32_t surf_tet_axis_b(uint32_t t) { return (0x489u >> (2u * t)) & 3u; } // 1, 2, 0, 2, 0, 1
// det(e_a, e_b, e_c) < 0: the odd permutations xzy, yxz, zyx
NRS_SURF_HD uint32_t surf_tet_negative(uint32_t t) { return (0x26u >> t) & 1u; }
// the four corner codes of tet t, 3 bits each, local corner 0 lowest
NRS_SURF_HD uint32_t surf_tet_corners(uint32_t t)
{
    const uint32_t c1 = 1u << surf_tet_axis_a(t), c2 = c1 | (1u << surf_tet_axis_b(t));
    return (c1 << 3) | (c2 << 6) | (7u << 9);
}

// ---- the 16 cases of a tetrahedron ------------------------------------------------------------------------------------------------------------
// m: bit c set when local corner c is inside.  The answer packs up to two triangles of three crossing edges each, an edge as
// (low corner | high corner << 2) in 4 bits, triangle 0 in bits 0..11 and triangle 1 in bits 12..23; the triangle count in bits 24..25;
// bit 26: the parity of the permutation (inside corners ascending, outside corners ascending).
//   one corner p inside, or one outside: the edges from p to the others, the others ascending
//   inside a < b, outside c < d: the quad ac, ad, bd, bc split along ac-bd into (ac, ad, bd) and (ac, bd, bc)
// Winding: with e the edge vectors from p, (v1 - v0) x (v2 - v0) . (e1 + e2 + e3) = (t1 t2 + t2 t3 + t3 t1) det(e1, e2, e3), and for the
// quad both normals are (d - c) x (b - a) / 4 at the edge midpoints, whose product with (c + d - a - b) is 2 det(b - a, c - a, d - a): the
// listed order has its right-hand normal from the inside corners to the outside ones exactly when the permutation above and the tet's
// permutation of the axes have the same parity, whatever the positions along the edges.  Otherwise the last two indices are swapped.
constexpr uint32_t surf_tet_edge(uint32_t p, uint32_t q) { return p < q ? (p | (q << 2)) : (q | (p << 2)); }
constexpr uint32_t surf_tet_case_build(uint32_t m)
{
    uint32_t in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0, inv = 0;
    for (uint32_t c = 0; c < 4; ++c) {
        if ((m >> c) & 1u) { inv += c - ni; in[ni++] = c; }
        else out[no++] = c;
    }
    uint32_t pk = (inv & 1u) << 26;
    if (ni == 1) pk |= surf_tet_edge(in[0], out[0]) | (surf_tet_edge(in[0], out[1]) << 4) | (surf_tet_edge(in[0], out[2]) << 8) | (1u << 24);
    else if (ni == 3) pk |= surf_tet_edge(in[0], out[0]) | (surf_tet_edge(in[1], out[0]) << 4) | (surf_tet_edge(in[2], out[0]) << 8) | (1u << 24);
    else if (ni == 2) {
        const uint32_t ac = surf_tet_edge(in[0], out[0]), ad = surf_tet_edge(in[0], out[1]), bd = surf_tet_edge(in[1], out[1]), bc = surf_tet_edge(in[1], out[0]);
        pk |= ac | (ad << 4) | (bd << 8) | (ac << 12) | (bd << 16) | (bc << 20) | (2u << 24);
    }
    return pk;
}
NRS_SURF_HD uint32_t surf_tet_case(uint32_t m)
{
#define NRS_SURF_CASE(x) case x: { constexpr uint32_t v = surf_tet_case_build(x); return v; }
    switch (m) {
        NRS_SURF_CASE(1) NRS_SURF_CASE(2) NRS_SURF_CASE(3) NRS_SURF_CASE(4) NRS_SURF_CASE(5) NRS_SURF_CASE(6) NRS_SURF_CASE(7)
        NRS_SURF_CASE(8) NRS_SURF_CASE(9) NRS_SURF_CASE(10) NRS_SURF_CASE(11) NRS_SURF_CASE(12) NRS_SURF_CASE(13) NRS_SURF_CASE(14)
    default: return 0u;
    }
#undef NRS_SURF_CASE
}
// triangles of the 16 cases, two bits each: 0 1 1 2 1 2 2 1 1 2 2 1 2 1 1 0
NRS_SURF_HD uint32_t surf_tet_count(uint32_t m) { return (0x16696994u >> (2u * m)) & 3u; }
// the inside bits of tet t's four corners from the cell's eight (bit = corner code)
NRS_SURF_HD uint32_t surf_tet_mask(uint32_t bits, uint32_t t)
{
    const uint32_t cc = surf_tet_corners(t);
    return (bits & 1u) | (((bits >> ((cc >> 3) & 7u)) & 1u) << 1) | (((bits >> ((cc >> 6) & 7u)) & 1u) << 2) | (((bits >> 7) & 1u) << 3);
}

// ---- the per-node routine ---------------------------------------------------------------------------------------------------------------------
// A node is inside when rho >= iso.  f[d]: the density of the node at offset d (a direction code; f[0] the node's own), read only where
// `have` says the node exists.  Returns the eight inside bits (bit = code; 0 for a node that does not exist).
template <typename R> NRS_SURF_HD uint32_t surf_inside_bits(const R f[8], R iso, uint32_t have)
{
    uint32_t bits = 0;
    NRS_SURF_UNROLL
    for (uint32_t d = 0; d < 8; ++d)
        if (!(d & ~have) && f[d] >= iso) bits |= 1u << d;
    return bits;
}
// the 7-bit mask of the owned edges that carry a vertex: the far node exists and the two ends differ in inside-ness; its popcount is the
// node's vertex count
NRS_SURF_HD uint32_t surf_node_mask(uint32_t bits, uint32_t have)
{
    uint32_t mask = 0;
    NRS_SURF_UNROLL
    for (uint32_t e = 0; e < 7; ++e) {
        const uint32_t d = surf_edge_dir(e);
        if (!(d & ~have) && (((bits >> d) ^ bits) & 1u)) mask |= 1u << e;
    }
    return mask;
}
NRS_SURF_HD uint32_t surf_popcount(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(x);
#else
    return (uint32_t)__builtin_popcount(x);
#endif
}
template <typename R> NRS_SURF_HD uint32_t surf_node_edges(const R f[8], R iso, uint32_t have, uint32_t *count)
{
    const uint32_t mask = surf_node_mask(surf_inside_bits<R>(f, iso, have), have);
    *count = surf_popcount(mask);
    return mask;
}
// the vertex of an owned edge, all in R: t = (iso - f0) / (f1 - f0) (f1 != f0: one end is >= iso, the other < iso), x = p0 + t (p1 - p0);
// the attributes are interpolated the same way
template <typename R> NRS_SURF_HD R surf_vertex_t(R iso, R f0, R f1) { return (iso - f0) / (f1 - f0); }
template <typename R> NRS_SURF_HD R surf_lerp(R a, R b, R t) { return a + t * (b - a); }

// ---- the per-cell routine ---------------------------------------------------------------------------------------------------------------------
// bits: the inside bits of the cell's eight corners.  Triangle count: 0..12.
NRS_SURF_HD uint32_t surf_cell_count(uint32_t bits)
{
    uint32_t n = 0;
    NRS_SURF_UNROLL
    for (uint32_t t = 0; t < 6; ++t) n += surf_tet_count(surf_tet_mask(bits, t));
    return n;
}
// emit(k, c0, e0, c1, e1, c2, e2) for the cell's k-th triangle, tets and triangles in their order: index i of the triangle is the vertex
// on edge number e_i of the node at the cell's corner c_i.  Returns the count.
template <typename Emit> NRS_SURF_HD uint32_t surf_cell_triangles(uint32_t bits, Emit &&emit)
{
    uint32_t n = 0;
    NRS_SURF_UNROLL
    for (uint32_t t = 0; t < 6; ++t) {
        const uint32_t cc = surf_tet_corners(t);
        const uint32_t pk = surf_tet_case(surf_tet_mask(bits, t));
        const uint32_t nt = (pk >> 24) & 3u;
        const bool swap = (((pk >> 26) & 1u) ^ surf_tet_negative(t)) != 0u;
        NRS_SURF_UNROLL
        for (uint32_t j = 0; j < 2; ++j) {
            if (j < nt) {
                uint32_t c[3], e[3];
                NRS_SURF_UNROLL
                for (uint32_t i = 0; i < 3; ++i) {
                    const uint32_t ed = (pk >> (12u * j + 4u * i)) & 15u;
                    const uint32_t lo = (cc >> (3u * (ed & 3u))) & 7u, hi = (cc >> (3u * (ed >> 2))) & 7u;
                    c[i] = lo;
                    e[i] = surf_dir_edge(hi ^ lo);
                }
                if (swap) emit(n, c[0], e[0], c[2], e[2], c[1], e[1]);
                else emit(n, c[0], e[0], c[1], e[1], c[2], e[2]);
                ++n;
            }
        }
    }
    return n;
}

} // namespace nrs
