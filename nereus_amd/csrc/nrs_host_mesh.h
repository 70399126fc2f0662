// nrs_host_mesh.h — the host decisions of the mesh sampling (include/nereus_hip.h "mesh sampling"; DESIGN.md "Mesh sampling"), written
// once: which meshes, rules and precisions are accepted and the refusal texts; the triangles gathered to nine doubles each; the plan
// of node batches; which halves of the field a rule needs; the selection predicate.  No HIP: the kernels (nrs_kernels_mesh.h), the
// owner of the device buffers (MeshSampler, nrs_mesh.h) and a plain host program (tests/host_mesh_main.cpp) call the same routines;
// NRS_MESH_HD is empty without hipcc.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "nrs_host_sample.h"

#if defined(__HIPCC__)
#define NRS_MESH_HD __host__ __device__ inline
#else
#define NRS_MESH_HD inline
#endif

namespace nrs {

constexpr uint64_t MESH_BATCH = 1ull << 22;          // nodes per launch: the per-node device buffers hold no more
constexpr uint64_t MESH_MAX_TRIANGLES = 1ull << 31;  // a triangle index is a uint32_t, 0xffffffff means none
constexpr uint32_t MESH_KNOWN_FLAGS = NRS_MESH_INSIDE | NRS_MESH_OUTSIDE | NRS_MESH_SNAP;

// ---- what a call may be given ------------------------------------------------------------------------------------------------------------
static inline int mesh_check_mesh(const nrs_mesh *m)
{
    if (!m) return fail(NRS_E_INVALID, "mesh is NULL");
    if (!m->vertices) return fail(NRS_E_INVALID, "mesh: vertices is NULL");
    if (!m->triangles) return fail(NRS_E_INVALID, "mesh: triangles is NULL");
    if (!m->nv) return fail(NRS_E_INVALID, "mesh: no vertices");
    if (!m->nt) return fail(NRS_E_INVALID, "mesh: no triangles");
    if (m->nt >= MESH_MAX_TRIANGLES) return fail(NRS_E_INVALID, "mesh: 2^31 triangles or more");
    for (uint64_t i = 0; i < 3 * m->nv; ++i)
        if (!std::isfinite(m->vertices[i])) return fail(NRS_E_INVALID, "mesh: a vertex coordinate is not finite");
    for (uint64_t i = 0; i < 3 * m->nt; ++i)
        if (m->triangles[i] >= m->nv) return fail(NRS_E_INVALID, "mesh: a triangle index is not below nv");
    return NRS_OK;
}
static inline int mesh_check_rule(const nrs_mesh_rule *r)
{
    if (!r) return fail(NRS_E_INVALID, "mesh rule is NULL");
    if (r->flags & ~MESH_KNOWN_FLAGS) return fail(NRS_E_INVALID, "mesh rule: flags has unknown bits");
    if (!(r->flags & (NRS_MESH_INSIDE | NRS_MESH_OUTSIDE))) return fail(NRS_E_INVALID, "mesh rule: flags names no side (NRS_MESH_INSIDE, NRS_MESH_OUTSIDE)");
    if (r->reserved) return fail(NRS_E_INVALID, "mesh rule: reserved must be 0");
    if (std::isnan(r->dmin) || r->dmin < 0.0) return fail(NRS_E_INVALID, "mesh rule: dmin must be >= 0");
    if (std::isnan(r->dmax)) return fail(NRS_E_INVALID, "mesh rule: dmax is NaN");
    if (r->dmax < r->dmin) return fail(NRS_E_INVALID, "mesh rule: dmax below dmin");
    return NRS_OK;
}
static inline int mesh_check_precision(int precision)
{
    if (precision != 32 && precision != 64) return fail(NRS_E_INVALID, "precision must be 32 or 64");
    return NRS_OK;
}
static inline int mesh_refuse_snap() { return fail(NRS_E_INVALID, "nrs_emit_mesh with NRS_MESH_SNAP (snapped points may coincide: they are wall samples, not fluid)"); }

// ---- the triangles as the kernel reads them: A, B, C of triangle t at tri9[9 t ...] -------------------------------------------------------
static inline void mesh_gather(const nrs_mesh &m, std::vector<double> &tri9)
{
    tri9.resize(9 * (size_t)m.nt);
    for (uint64_t t = 0; t < m.nt; ++t)
        for (int c = 0; c < 3; ++c) {
            const uint64_t v = m.triangles[3 * t + c];
            for (int a = 0; a < 3; ++a) tri9[9 * t + 3 * c + a] = m.vertices[3 * v + a];
        }
}

// ---- the plan: batch b covers the nodes [b MESH_BATCH, min(N, (b + 1) MESH_BATCH)) ---------------------------------------------------------
static inline uint64_t mesh_batches(uint64_t nodes) { return (nodes + MESH_BATCH - 1) / MESH_BATCH; }
static inline void mesh_batch(uint64_t nodes, uint64_t b, uint64_t &first, uint32_t &count)
{
    first = b * MESH_BATCH;
    const uint64_t left = nodes - first;
    count = (uint32_t)(left < MESH_BATCH ? left : MESH_BATCH);
}

// ---- the selection ---------------------------------------------------------------------------------------------------------------------------
// both sides selected: the winding number decides nothing; no distance bound and no snap: the distance decides nothing (it is
// evaluated all the same when the winding is not: a launch computes at least one half)
static inline bool mesh_rule_needs_winding(const nrs_mesh_rule &r) { return (r.flags & (NRS_MESH_INSIDE | NRS_MESH_OUTSIDE)) != (NRS_MESH_INSIDE | NRS_MESH_OUTSIDE); }
static inline bool mesh_rule_needs_distance(const nrs_mesh_rule &r)
{
    return r.dmin > 0.0 || r.dmax < INFINITY || (r.flags & NRS_MESH_SNAP) || !mesh_rule_needs_winding(r);
}
// the rule as the kernels get it; the squares are formed once, in double
struct MeshSelect {
    double dmin2, dmax2;
    uint32_t flags;
    uint32_t useW, useD;
};
static inline MeshSelect mesh_select_from(const nrs_mesh_rule &r)
{
    MeshSelect s;
    s.dmin2 = r.dmin * r.dmin; s.dmax2 = r.dmax * r.dmax; s.flags = r.flags;
    s.useW = mesh_rule_needs_winding(r) ? 1u : 0u;
    s.useD = mesh_rule_needs_distance(r) ? 1u : 0u;
    return s;
}
// w, d2: read only where the rule uses them
NRS_MESH_HD bool mesh_selected(const MeshSelect &s, double w, double d2)
{
    if (s.useW && !((s.flags & NRS_MESH_INSIDE) ? w > 0.5 : w <= 0.5)) return false; // (exactly one side is named)
    if (s.useD && !(s.dmin2 <= d2 && d2 <= s.dmax2)) return false;
    return true;
}

} // namespace nrs
