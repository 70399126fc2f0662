// nrs_mesh.h — the owner of everything the mesh sampling keeps on the device (DESIGN.md "Mesh sampling"): the gathered triangles, the
// field of one node batch, the workgroup totals and the header of the selection, the selected node indices (and snapped points), the
// particles of nrs_mesh_particles.  Nothing is allocated before the first call; release() frees everything.  It depends on neither a
// context nor a precision: nrs_mesh_field and nrs_mesh_particles hold one for the length of the call, a context (nrs_ctx_impl.h) holds one
// for nrs_emit_mesh and releases it before the call returns.  nrs_mesh.hip defines the routines and is the one translation unit that
// compiles the kernels (nrs_kernels_mesh.h); this header includes no kernel.  The host decisions are nrs_host_mesh.h's.
#pragma once
#include "nrs_ctx_base.h"
#include "nrs_host_mesh.h"

namespace nrs {

struct MeshSampler {
    // the (checked) mesh's triangles to the device, on `stream`; waits (the gathered host copy goes on return)
    int upload(const nrs_mesh &mesh, hipStream_t stream);
    // the field on the `nodes` nodes of L, batch by batch, into the HOST arrays that are not null; waits
    int field(const Lattice &L, uint64_t nodes, double *winding, double *dist2, uint32_t *nearest, double *closest3, hipStream_t stream);
    // the selection of rule r among the nodes of L: at most `limit` node indices (with NRS_MESH_SNAP also their closest points) are
    // kept on the device, in linear index order; *count is the number selected, read back with one wait at the end
    int select(const Lattice &L, uint64_t nodes, const nrs_mesh_rule &r, uint64_t limit, hipStream_t stream, uint64_t *count);
    // the first `count` (<= limit) selected nodes as SVec4 of the precision into the HOST array pos4; waits
    int positions(int precision, const Lattice &L, uint64_t count, void *pos4, hipStream_t stream);
    // the selected node indices of the last select(), for nrs_emit_mesh's append kernel
    const uint32_t *selected() const { return selIdx.as<uint32_t>(); }

    void release()
    {
        for (DevBuf *b : {&tri, &w, &d2, &near, &q, &blockTot, &hdr, &selIdx, &selQ, &pos}) b->release();
        nt = 0;
        snapped = false;
    }

private:
    int batch_field(const Lattice &L, uint64_t first, uint32_t m, bool wind, bool dist, hipStream_t stream);
    DevBuf tri;             // 9 doubles per triangle
    uint32_t nt = 0;
    DevBuf w, d2, near, q;  // the field of one batch: double, double, uint32_t, 3 doubles per node
    DevBuf blockTot, hdr;   // selected nodes per workgroup of one batch, scanned in place; MeshHeader
    DevBuf selIdx, selQ;    // uint32_t / 3 doubles per selected node
    bool snapped = false;   // selQ is in use
    DevBuf pos;             // SVec4 per selected node (nrs_mesh_particles)
};

} // namespace nrs
