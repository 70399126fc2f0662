// nrs_surface_mesher.h — the owner of everything the surface extraction keeps on the device (DESIGN.md "Surface extraction"): the
// workgroup totals and their scan, the per-node vertex offsets and edge masks, and the mesh itself — vertices, triangles and the two
// optional attribute arrays.  Nothing is allocated before the first extract; everything grows as needed and nrs_surface_release frees it.
// It depends on neither the solver, the kernel set nor the sampler: the owner of the read-only add-ons (FluidReaders, nrs_readers.h) holds
// one next to its FieldSampler and hands it the device pointers of a sampled lattice.  nrs_surface.hip defines extract() and is the one translation unit that
// compiles the kernels (nrs_kernels_surface.h), for float and double; this header includes no kernel.  The host decisions — what is
// accepted, sizes, which result an id means — are in nrs_host_surface.h.
#pragma once
#include "nrs_ctx_base.h"
#include "nrs_host_surface.h"

namespace nrs {

// one sampled lattice on the device: SReal[nodes] density and, or null, SVec4[nodes] gradient / velocity (precision 32 or 64)
struct SurfaceInput {
    Lattice L;
    uint64_t nodes;
    double iso;
    int precision;
    const void *dens, *grad, *vel;
};

struct SurfaceMesher {
    SurfaceLast last; // what the mesh buffers hold

    // Meshes `in` on `stream`: count, scan, then ONE wait for the stream and an eight-byte read-back of (V, T) to size the outputs, then
    // the two emit launches (not waited for).  On success the buffers hold the mesh; `last` is the caller's to set.
    int extract(const SurfaceInput &in, hipStream_t stream, uint64_t *V, uint64_t *T);

    void *result(uint32_t which) const
    {
        switch (which) {
        case NRS_MESH_VERTICES: return vert.p;
        case NRS_MESH_TRIANGLES: return tri.p;
        case NRS_MESH_GRADIENT: return vgrad.p;
        case NRS_MESH_VELOCITY: return vvel.p;
        default: return nullptr;
        }
    }

    // nrs_surface_release: every buffer goes (the caller has drained the stream); the next extract allocates again
    void release()
    {
        for (DevBuf *b : {&blockTot, &nodeOff, &nodeMask, &vert, &tri, &vgrad, &vvel}) b->release();
        last = SurfaceLast();
    }

private:
    template <typename R> int extract_t(const SurfaceInput &in, hipStream_t stream, uint64_t *V, uint64_t *T);
    DevBuf blockTot;          // uint2 per workgroup of the lattice kernels + 1: (vertices, triangles), scanned in place; the last is (V, T)
    DevBuf nodeOff, nodeMask; // per node: number of its first vertex (uint32), mask of its edges that carry one (uint8)
    DevBuf vert, tri;         // SVec4[V], uint32[3 T]
    DevBuf vgrad, vvel;       // SVec4[V] each, when asked for
};

} // namespace nrs
