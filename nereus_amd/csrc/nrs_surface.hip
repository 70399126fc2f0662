// nrs_surface.hip — the surface extraction's launches (nrs_surface_mesher.h has the owner, nrs_kernels_surface.h the kernels): the one
// translation unit of libnereus_hip.so that compiles them, once for float and once for double.
#include "nrs_surface_mesher.h"

#include "nrs_kernels_surface.h"

namespace nrs {

template <typename R> int SurfaceMesher::extract_t(const SurfaceInput &in, hipStream_t stream, uint64_t *V, uint64_t *T)
{
    typedef typename SurfVec4<R>::type T4;
    const uint32_t nodes = (uint32_t)in.nodes; // <= 2^27 (surface_check_lattice)
    const uint32_t nb = (nodes + SURF_BLOCK - 1) / SURF_BLOCK;
    const R iso = (R)in.iso;
    const R *dens = (const R *)in.dens;
    NRSCHK(blockTot.alloc(sizeof(uint2) * ((size_t)nb + 1)));
    NRSCHK(nodeOff.alloc(4 * (size_t)nodes));
    NRSCHK(nodeMask.alloc((size_t)nodes));
    uint2 *tot = blockTot.as<uint2>();
    hipLaunchKernelGGL((k_surf_count<R>), dim3(nb), dim3(SURF_BLOCK), 0, stream, dens, in.L, iso, nodes, tot);
    hipLaunchKernelGGL(k_surf_scan, dim3(1), dim3(SCAN_BLOCK), 0, stream, tot, nb);
    HIPCHK(hipGetLastError());
    uint32_t vt[2] = {0u, 0u};
    HIPCHK(hipMemcpyAsync(vt, tot + nb, sizeof(vt), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    *V = vt[0];
    *T = vt[1];
    if (!vt[0] && !vt[1]) return NRS_OK;
    NRSCHK(vert.alloc(sizeof(T4) * (size_t)vt[0]));
    NRSCHK(tri.alloc(12 * (size_t)vt[1]));
    if (in.grad) NRSCHK(vgrad.alloc(sizeof(T4) * (size_t)vt[0]));
    if (in.vel) NRSCHK(vvel.alloc(sizeof(T4) * (size_t)vt[0]));
    const SurfVertexOut<R> O{nodeOff.as<uint32_t>(), nodeMask.as<uint8_t>(), vert.as<T4>(), in.grad ? vgrad.as<T4>() : nullptr, in.vel ? vvel.as<T4>() : nullptr};
    hipLaunchKernelGGL((k_surf_vertices<R>), dim3(nb), dim3(SURF_BLOCK), 0, stream, dens, (const T4 *)in.grad, (const T4 *)in.vel, in.L, iso, nodes,
                       (const uint2 *)tot, O);
    hipLaunchKernelGGL((k_surf_triangles<R>), dim3(nb), dim3(SURF_BLOCK), 0, stream, dens, in.L, iso, nodes, (const uint2 *)tot,
                       (const uint32_t *)nodeOff.as<uint32_t>(), (const uint8_t *)nodeMask.as<uint8_t>(), tri.as<uint32_t>());
    HIPCHK(hipGetLastError());
    return NRS_OK;
}

int SurfaceMesher::extract(const SurfaceInput &in, hipStream_t stream, uint64_t *V, uint64_t *T)
{
    return in.precision == 64 ? extract_t<double>(in, stream, V, T) : extract_t<float>(in, stream, V, T);
}

} // namespace nrs
