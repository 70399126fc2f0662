// nrs_aniso.hip — the launches of the anisotropic surface reconstruction (nrs_aniso.h has the owner, nrs_kernels_aniso.h the kernels): the
// one translation unit of libnereus_hip.so that compiles them, once for float and once for double.
#include "nrs_aniso.h"

#include "nrs_kernels_aniso.h"

namespace nrs {

template <typename R>
int AnisoSurface::records(const Params<R> &P, const GridView<R> &G, const AnisoConfig &cfg, const typename Vec4T<R>::type *sPos,
                          const uint32_t *sIndex, uint32_t n, hipStream_t stream)
{
    typedef typename Vec4T<R>::type T4;
    if (!n) return NRS_OK;
    NRSCHK(center.alloc(sizeof(T4) * (size_t)n));
    NRSCHK(g.alloc(2 * sizeof(T4) * (size_t)n));
    NRSCHK(count.alloc(4 * (size_t)n));
    NRSCHK(index.alloc(4 * (size_t)n));
    const AnisoOut<R> O{center.as<T4>(), g.as<T4>(), count.as<uint32_t>(), index.as<uint32_t>()};
    hipLaunchKernelGGL((k_aniso_records<R>), dim3(nblocks(n)), dim3(BLOCK), 0, stream, P, G, aniso_consts<R>(cfg), sPos, sIndex, O, n);
    HIPCHK(hipGetLastError());
    return NRS_OK;
}

template <typename R>
int AnisoSurface::lattice(const Params<R> &P, const GridView<R> &G, const typename Vec4T<R>::type *sVel, const Lattice &L, uint64_t m, void *dens,
                          void *grad, void *vel, hipStream_t stream)
{
    typedef typename Vec4T<R>::type T4;
    if (!m) return NRS_OK;
    hipLaunchKernelGGL((k_aniso_lattice<R>), dim3(nblocks(m)), dim3(BLOCK), 0, stream, P, G, (const T4 *)center.as<T4>(), (const T4 *)g.as<T4>(), sVel, L,
                       (R *)dens, (T4 *)grad, (T4 *)vel, (uint32_t)m);
    HIPCHK(hipGetLastError());
    return NRS_OK;
}

template int AnisoSurface::records<float>(const Params<float> &, const GridView<float> &, const AnisoConfig &, const float4 *, const uint32_t *, uint32_t, hipStream_t);
template int AnisoSurface::records<double>(const Params<double> &, const GridView<double> &, const AnisoConfig &, const double4 *, const uint32_t *, uint32_t, hipStream_t);
template int AnisoSurface::lattice<float>(const Params<float> &, const GridView<float> &, const float4 *, const Lattice &, uint64_t, void *, void *, void *, hipStream_t);
template int AnisoSurface::lattice<double>(const Params<double> &, const GridView<double> &, const double4 *, const Lattice &, uint64_t, void *, void *, void *, hipStream_t);

} // namespace nrs
