// nrs_track.h — the owner of what particle tracking keeps (DESIGN.md "Particle identity and attributes"): per fluid particle an id, a
// birth stamp and, with NRS_TRACK_ATTR, one SVec4 of user data, double-buffered like the particle arrays they follow; the id counter and
// the emit values on the host; the inverse map of the last nrs_track_locate and the density scratch of nrs_track_diffuse.  Nothing is
// allocated before nrs_track_enable.  Like the sources and sinks it is the context's own member: the context (nrs_ctx_impl.h) refuses
// what has to be refused, says where in its arrays something happened and swaps when its own arrays swap.  The host decisions are
// nrs_host_track.h's, the kernels nrs_kernels_track.h's.
#pragma once
#include "nrs_ctx_base.h"
#include "nrs_host_track.h"
#include "nrs_kernels_track.h"

namespace nrs {

struct TrackSystem {
    bool on = false;
    uint32_t flags = 0;
    TrackIds ids;
    double emitValue[TRACK_EMIT_VALUES][4] = {}; // [0]: slot -1, [1 + s]: emitter s
    bool haveLocate = false;
    uint64_t located = 0;

    bool attr() const { return (flags & NRS_TRACK_ATTR) != 0; }
    const double *emit_value(int32_t slot) const { return emitValue[slot + 1]; }
    // the arrays of the current order / the other set (a step's gather, a cull and a diffusion write there, then swap)
    template <typename R> TrackView<R> cur() const { return TrackView<R>{idA.as<uint32_t>(), birthA.as<uint32_t>(), (typename Vec4T<R>::type *)recA.p}; }
    template <typename R> TrackView<R> other() const { return TrackView<R>{idB.as<uint32_t>(), birthB.as<uint32_t>(), (typename Vec4T<R>::type *)recB.p}; }
    void swap()
    {
        std::swap(idA.p, idB.p);
        std::swap(birthA.p, birthB.p);
        std::swap(recA.p, recB.p);
    }

    // nrs_track_enable (checked): the n particles present are numbered 0 .. n-1 in the current order, birth 0, record zeros
    template <typename R> int enable(uint32_t newFlags, uint64_t cap, uint64_t n, hipStream_t stream)
    {
        typedef typename Vec4T<R>::type T4;
        if (on) HIPCHK(hipStreamSynchronize(stream)); // queued launches may still use a record buffer that goes
        const bool rec = (newFlags & NRS_TRACK_ATTR) != 0;
        NRSCHK(idA.alloc(4 * cap)); NRSCHK(idB.alloc(4 * cap)); NRSCHK(birthA.alloc(4 * cap)); NRSCHK(birthB.alloc(4 * cap));
        if (rec) { NRSCHK(recA.alloc(sizeof(T4) * cap)); NRSCHK(recB.alloc(sizeof(T4) * cap)); }
        else { recA.release(); recB.release(); }
        on = true;
        flags = newFlags;
        ids = TrackIds();
        std::memset(emitValue, 0, sizeof(emitValue));
        haveLocate = false;
        located = 0;
        uint32_t firstId = 0;
        NRSCHK(ids.reserve(n, &firstId));
        const double zero[4] = {0.0, 0.0, 0.0, 0.0};
        return fill<R>(0, n, firstId, 0u, zero, stream);
    }
    // nrs_track_disable: the stream is drained, every buffer goes
    int disable(hipStream_t stream)
    {
        if (on) HIPCHK(hipStreamSynchronize(stream));
        for (DevBuf *b : {&idA, &idB, &birthA, &birthB, &recA, &recB, &slotOf, &rho}) b->release();
        on = false;
        flags = 0;
        ids = TrackIds();
        haveLocate = false;
        located = 0;
        return NRS_OK;
    }

    // the one launch behind a step's reorder: other[s] = cur[index[s]]; the context swaps at the end of the step
    template <typename R> void gather(const uint32_t *index, uint32_t n, hipStream_t stream)
    {
        hipLaunchKernelGGL((k_track_gather<R>), dim3(nblocks(n)), dim3(BLOCK), 0, stream, index, cur<R>(), other<R>(), n);
    }
    // slots [first, first + count) of the current order are new particles; enqueues
    template <typename R> int fill(uint64_t first, uint64_t count, uint32_t firstId, uint32_t birth, const double val[4], hipStream_t stream)
    {
        if (!count) return NRS_OK;
        hipLaunchKernelGGL((k_track_fill<R>), dim3(nblocks(count)), dim3(BLOCK), 0, stream, cur<R>(), (uint32_t)first, (uint32_t)count, firstId, birth,
                           mk4_host<R>(val));
        HIPCHK(hipGetLastError());
        return NRS_OK;
    }
    // nrs_track_upload (checked): waits, the caller may reuse its memory on return
    template <typename R> int upload(uint32_t which, const void *src, uint64_t first, uint64_t count, hipStream_t stream)
    {
        typedef typename Vec4T<R>::type T4;
        if (!count) return NRS_OK;
        if (which == NRS_TRACK_ID) HIPCHK(hipMemcpyAsync(idA.as<uint32_t>() + first, src, 4 * count, hipMemcpyHostToDevice, stream));
        else if (which == NRS_TRACK_BIRTH) HIPCHK(hipMemcpyAsync(birthA.as<uint32_t>() + first, src, 4 * count, hipMemcpyHostToDevice, stream));
        else HIPCHK(hipMemcpyAsync(recA.as<T4>() + first, src, sizeof(T4) * count, hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return NRS_OK;
    }
    // nrs_track_locate (checked): enqueues
    int locate(uint64_t firstId, uint64_t count, uint64_t n, hipStream_t stream)
    {
        haveLocate = false;
        NRSCHK(slotOf.alloc(4 * count));
        if (count) HIPCHK(hipMemsetAsync(slotOf.p, 0xff, 4 * count, stream));
        if (count && n) {
            hipLaunchKernelGGL(k_track_locate, dim3(nblocks(n)), dim3(BLOCK), 0, stream, (const uint32_t *)idA.as<uint32_t>(), (uint32_t)n, firstId, (uint32_t)count,
                               slotOf.as<uint32_t>());
            HIPCHK(hipGetLastError());
        }
        haveLocate = true;
        located = count;
        return NRS_OK;
    }
    void *result(uint32_t which) const
    {
        switch (which) {
        case NRS_TRACK_ID: return idA.p;
        case NRS_TRACK_BIRTH: return birthA.p;
        case NRS_TRACK_ATTRIBUTE: return recA.p;
        case NRS_TRACK_SLOT_OF: return slotOf.p;
        default: return nullptr;
        }
    }
    // nrs_track_diffuse (checked) on the sampler's grid G of the n sorted particles sPos, sIndex their places in the current order:
    // the density at the particles (walls: with the boundary term), the diffusion into the other record buffer, the swap.  Enqueues.
    template <typename R, int KSET>
    int diffuse(const Params<R> &P, const GridView<R> &G, bool walls, const typename Vec4T<R>::type *sPos, const typename Vec4T<R>::type *sVel,
                const uint32_t *sIndex, uint32_t n, const double kappa[4], double dt, hipStream_t stream)
    {
        typedef typename Vec4T<R>::type T4;
        if (!n) return NRS_OK;
        NRSCHK(rho.alloc(sizeof(R) * (size_t)n));
        const SampleOut<R> O{rho.as<R>(), nullptr, nullptr, nullptr};
        const dim3 g(nblocks(n)), b(BLOCK);
        if (walls) hipLaunchKernelGGL((k_sample_points<R, KSET, true>), g, b, 0, stream, P, G, sPos, sVel, sPos, Lattice(), O, (uint32_t)(NRS_FIELD_DENSITY | NRS_FIELD_WALLS), n);
        else hipLaunchKernelGGL((k_sample_points<R, KSET, false>), g, b, 0, stream, P, G, sPos, sVel, sPos, Lattice(), O, (uint32_t)NRS_FIELD_DENSITY, n);
        TrackDiffuseArgs<R> A;
        for (int c = 0; c < 4; ++c) A.kappa[c] = (R)kappa[c];
        A.dt = (R)dt;
        hipLaunchKernelGGL((k_track_diffuse<R, KSET>), g, b, 0, stream, P, G, sPos, sIndex, (const R *)rho.as<R>(), (const T4 *)recA.as<T4>(), recB.as<T4>(), A, n);
        HIPCHK(hipGetLastError());
        std::swap(recA.p, recB.p);
        return NRS_OK;
    }

private:
    template <typename R> static typename Vec4T<R>::type mk4_host(const double v[4])
    {
        typename Vec4T<R>::type o;
        o.x = (R)v[0]; o.y = (R)v[1]; o.z = (R)v[2]; o.w = (R)v[3];
        return o;
    }
    DevBuf idA, idB, birthA, birthB, recA, recB; // A: the current order
    DevBuf slotOf;                              // uint32[located] of the last nrs_track_locate
    DevBuf rho;                                 // nrs_track_diffuse: the density at the sorted particles
};

} // namespace nrs
