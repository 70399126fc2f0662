// nrs_aniso.h — the owner of everything the anisotropic surface reconstruction keeps on the device (DESIGN.md "Anisotropic kernels"): the
// per-particle records of pass A.  Nothing is allocated before the first build; everything grows as needed and nrs_aniso_release frees
// it.  It depends on neither the solver nor the kernel set: the owner of the read-only add-ons (FluidReaders, nrs_readers.h) holds one
// next to its sampler and mesher, hands it the sampler's grid and sorted arrays and, for pass B, the sampler's result arrays.
// nrs_aniso.hip defines records() and lattice() and is the one translation unit that compiles the kernels (nrs_kernels_aniso.h), for
// float and double; this header includes no kernel.  The host decisions and the finishing routine are in nrs_host_aniso.h.
#pragma once
#include "nrs_ctx_base.h"
#include "nrs_host_aniso.h"
#include "nrs_kernels_ref.h"

namespace nrs {

struct AnisoSurface {
    AnisoLast last; // what the record buffers hold

    // Pass A on `stream` (enqueued, not waited for) for the n sorted particles of the grid G: sPos the sorted positions, sIndex the sort
    // values.  `last` is the caller's to set.
    template <typename R>
    int records(const Params<R> &P, const GridView<R> &G, const AnisoConfig &cfg, const typename Vec4T<R>::type *sPos, const uint32_t *sIndex,
                uint32_t n, hipStream_t stream);
    // Pass B on the m nodes of L from the records of the last records() call (the same grid): dens (SReal[m]) and, unless null,
    // grad / vel (SVec4[m]); sVel: the sorted velocities
    template <typename R>
    int lattice(const Params<R> &P, const GridView<R> &G, const typename Vec4T<R>::type *sVel, const Lattice &L, uint64_t m, void *dens,
                void *grad, void *vel, hipStream_t stream);

    void *result(uint32_t which) const
    {
        switch (which) {
        case NRS_ANISO_CENTER: return center.p;
        case NRS_ANISO_G: return g.p;
        case NRS_ANISO_COUNT: return count.p;
        case NRS_ANISO_INDEX: return index.p;
        default: return nullptr;
        }
    }

    // nrs_aniso_release: every buffer goes (the caller has drained the stream); the next build allocates again
    void release()
    {
        for (DevBuf *b : {&center, &g, &count, &index}) b->release();
        last = AnisoLast();
    }

private:
    DevBuf center, g;    // SVec4[n], SVec4[2n]
    DevBuf count, index; // uint32[n] each
};

} // namespace nrs
