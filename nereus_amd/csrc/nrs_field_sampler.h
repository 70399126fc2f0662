// nrs_field_sampler.h — the owner of everything the field sampler keeps on the device (DESIGN.md "Field sampling"): its (hash, index)
// pairs and sort workspace, its sorted copy of the fluid's positions and velocities, its own fluid cell table, the uploaded query
// points and the four result arrays.  Nothing is allocated before the first sample call; everything grows as needed and
// nrs_sample_release frees it.  It depends on neither the solver nor the kernel set: FluidReaders (nrs_readers.h) holds one, tells it
// the particle state to build from (build_grid) and launches the gather (nrs_kernels_sample.h) on its views.
//
// It READS the context's current positions and velocities and writes only its own buffers: the context's cell table, sort stage and
// array state never see a sample call.  The host decisions — what is accepted, when the grid is rebuilt, which result a field id means —
// are in nrs_host_sample.h.
#pragma once
#include "nrs_ctx_base.h"
#include "nrs_host_grid.h"
#include "nrs_host_sample.h"
#include "nrs_host_state.h"
#include "nrs_kernels_sample.h"
#include "nrs_sort.h"

namespace nrs {

struct FieldSampler {
    SampleCache cache; // which particle state the grid below was built from; nrs_sample_builds
    SampleLast last;   // what the result arrays hold

    // ---- views -----------------------------------------------------------------------------------------------------------------------
    uint32_t sorted_count() const { return builtN; }
    template <typename T4> const T4 *sorted_pos() const { return sPos.as<T4>(); }
    template <typename T4> const T4 *sorted_vel() const { return sVel.as<T4>(); }
    const uint32_t *cell_start() const { return cellStart.as<uint32_t>(); }
    const uint32_t *cell_end() const { return cellEnd.as<uint32_t>(); }
    uint32_t *err_word() const { return err.as<uint32_t>(); }
    const uint32_t *sorted_index() const { return valCur; } // slot -> the particle's index in the arrays the grid was built from
    template <typename T4> const T4 *query_points() const { return points.as<T4>(); }
    void *result(uint32_t field) const
    {
        switch (field) {
        case NRS_FIELD_DENSITY: return rDens.p;
        case NRS_FIELD_GRADIENT: return rGrad.p;
        case NRS_FIELD_VELOCITY: return rVel.p;
        case NRS_FIELD_COUNT: return rCount.p;
        default: return nullptr;
        }
    }

    // ---- the particle grid: k_hash -> sort_pairs_plain -> k_reorder on the sampler's own buffers ---------------------------------------
    // pos / vel: the context's current arrays (n live particles), P its kernel parameters.  Enqueues on `stream`; waits for nothing
    // unless a buffer has to grow.
    template <typename R>
    int build_grid(const Params<R> &P, const typename Vec4T<R>::type *pos, const typename Vec4T<R>::type *vel, uint64_t n, hipStream_t stream)
    {
        typedef typename Vec4T<R>::type T4;
        const uint32_t N = (uint32_t)n, C = P.numCells;
        if (!err.p) {
            NRSCHK(err.alloc(4));
            HIPCHK(hipMemsetAsync(err.p, 0, 4, stream));
        }
        // an all-EMPTY cell table: only the cells the last build touched (its sorted keys name them) where the table is big and mostly
        // empty, a full reset otherwise.  First, while the old keys are still there: a buffer that grows below frees them.
        if ((size_t)C * 4 > cellStart.bytes || C != tableCells) {
            NRSCHK(cellStart.alloc((size_t)C * 4));
            NRSCHK(cellEnd.alloc((size_t)C * 4));
            HIPCHK(hipMemsetAsync(cellStart.p, 0xff, (size_t)C * 4, stream));
            HIPCHK(hipMemsetAsync(cellEnd.p, 0, (size_t)C * 4, stream));
            tableCells = C;
        } else if (builtN && sparse_cell_table(C, builtN)) {
            hipLaunchKernelGGL(k_clear_cells, dim3(nblocks(builtN)), dim3(BLOCK), 0, stream, keyCur, cellStart.as<uint32_t>(), builtN);
        } else if (builtN) {
            HIPCHK(hipMemsetAsync(cellStart.p, 0xff, (size_t)C * 4, stream));
        }
        builtN = 0;
        if (!N) return NRS_OK;
        NRSCHK(key.alloc(4 * (size_t)N)); NRSCHK(keyAlt.alloc(4 * (size_t)N)); NRSCHK(val.alloc(4 * (size_t)N)); NRSCHK(valAlt.alloc(4 * (size_t)N));
        NRSCHK(sPos.alloc(sizeof(T4) * (size_t)N)); NRSCHK(sVel.alloc(sizeof(T4) * (size_t)N));
        hipLaunchKernelGGL((k_hash<R>), dim3(nblocks(N)), dim3(BLOCK), 0, stream, P, pos, key.as<uint32_t>(), val.as<uint32_t>(), N);
        PairBuffers kv{key.as<uint32_t>(), keyAlt.as<uint32_t>(), val.as<uint32_t>(), valAlt.as<uint32_t>()};
        const unsigned bits = sort_key_bits(C);
        size_t tmp = 0;
        HIPCHK(sort_pairs_plain(nullptr, tmp, kv, (size_t)N, bits, stream));
        NRSCHK(sortTmp.alloc(tmp));
        HIPCHK(sort_pairs_plain(sortTmp.p, tmp, kv, (size_t)N, bits, stream));
        keyCur = kv.key;
        valCur = kv.val;
        hipLaunchKernelGGL((k_reorder<R>), dim3(nblocks(N)), dim3(BLOCK), 0, stream, (const uint32_t *)kv.key, (const uint32_t *)kv.val, pos, vel,
                           (const R *)nullptr, sPos.as<T4>(), sVel.as<T4>(), (R *)nullptr, cellStart.as<uint32_t>(), cellEnd.as<uint32_t>(),
                           (uint32_t *)nullptr, N, (const uint32_t *)nullptr, (uint32_t *)nullptr, (unsigned long long *)nullptr, QuantCfg{},
                           (qword_t *)nullptr);
        HIPCHK(hipGetLastError());
        builtN = N;
        return NRS_OK;
    }

    // ---- the queries and the results of a call ---------------------------------------------------------------------------------------------
    // m points of `bytes` each, from the caller's host memory through a pinned staging buffer: the caller may reuse its memory on
    // return, and nothing waits for the stream (only for the previous call's copy out of the same staging buffer)
    int upload_points(const void *points4, uint64_t m, size_t bytes, hipStream_t stream)
    {
        const size_t total = (size_t)m * bytes;
        if (stagedEvent.e) HIPCHK(hipEventSynchronize(stagedEvent));
        else HIPCHK(hipEventCreateWithFlags(&stagedEvent.e, hipEventDisableTiming));
        if (total > stagedBytes) {
            staged.release();
            stagedBytes = 0;
            HIPCHK(hipHostMalloc((void **)&staged.p, total, hipHostMallocDefault));
            stagedBytes = total;
        }
        NRSCHK(points.alloc(total));
        std::memcpy(staged.p, points4, total);
        HIPCHK(hipMemcpyAsync(points.p, staged.p, total, hipMemcpyHostToDevice, stream));
        HIPCHK(hipEventRecord(stagedEvent, stream));
        return NRS_OK;
    }
    // the result arrays `fields` asks for, for m queries of a build whose SReal has `real` bytes
    int ensure_results(uint32_t fields, uint64_t m, size_t real)
    {
        if (fields & NRS_FIELD_DENSITY) NRSCHK(rDens.alloc(real * m));
        if (fields & NRS_FIELD_GRADIENT) NRSCHK(rGrad.alloc(4 * real * m));
        if (fields & NRS_FIELD_VELOCITY) NRSCHK(rVel.alloc(4 * real * m));
        if (fields & NRS_FIELD_COUNT) NRSCHK(rCount.alloc(4 * m));
        return NRS_OK;
    }

    // nrs_sample_release: every buffer goes (the caller has drained the stream); the next sample call allocates again
    void release()
    {
        for (DevBuf *b : {&key, &keyAlt, &val, &valAlt, &sortTmp, &sPos, &sVel, &cellStart, &cellEnd, &points, &rDens, &rGrad, &rVel, &rCount, &err}) b->release();
        staged.release();
        stagedBytes = 0;
        stagedEvent.release();
        keyCur = valCur = nullptr;
        builtN = 0;
        tableCells = 0;
        cache.dropped();
        last = SampleLast();
    }

private:
    DevBuf key, keyAlt, val, valAlt, sortTmp; // the (hash, index) pairs of the last build and the sort's workspace
    uint32_t *keyCur = nullptr;               // whichever of key / keyAlt the sort left the sorted hashes in
    uint32_t *valCur = nullptr;               // ... and of val / valAlt the sorted indices
    DevBuf sPos, sVel;                        // the fluid in sorted order
    DevBuf cellStart, cellEnd;                // the sampler's own fluid cell table
    uint32_t builtN = 0;                      // particles the table describes (0: the table is all-EMPTY)
    uint32_t tableCells = 0;                  // cells the table was reset for
    DevBuf points;                            // the uploaded query points of the last nrs_sample_points
    PinnedBuf<unsigned char> staged;          // ... and the pinned buffer they travel through
    size_t stagedBytes = 0;
    Event stagedEvent;
    DevBuf rDens, rGrad, rVel, rCount;        // results of the last call
    DevBuf err;                               // run guard of the gather (GridView::err)
};

} // namespace nrs
