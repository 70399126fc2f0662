// nrs_host_snapshot.h — asynchronous snapshots for a viewer (include/nereus_hip.h: nrs_snapshot_*): two slots, each a device staging
// copy made in stream order and a page-locked host landing filled on a copy stream of the ring's own.  The ring needs the source
// arrays and an element size, nothing else of the context.
#pragma once
#include "nrs_ctx_base.h"

namespace nrs {

struct SnapshotRing {
    struct Snap {
        DevBuf dPos, dVel;
        PinnedBuf<void> hPos, hVel;
        Event staged, done;
        uint64_t n = 0, step = 0;
        bool withVel = false, pending = false;
    };
    Snap snaps[2];
    int head = 0, tail = 0; // next slot to fill / oldest pending slot
    hipStream_t copyStream = nullptr;

    ~SnapshotRing() { release(); }
    void release()
    {
        for (Snap &sn : snaps) {
            if (sn.pending && sn.done) (void)hipEventSynchronize(sn.done);
            sn = Snap();
        }
        if (copyStream) (void)hipStreamDestroy(copyStream);
        copyStream = nullptr;
    }
    // pos / vel: n live elements of elem bytes each, in arrays of cap elements; the copies are ordered behind `stream`
    int begin(const void *pos, const void *vel, size_t elem, uint64_t cap, uint64_t n, uint64_t step, hipStream_t stream)
    {
        const bool withVel = vel != nullptr;
        if (!copyStream) HIPCHK(hipStreamCreateWithFlags(&copyStream, hipStreamNonBlocking));
        Snap &sn = snaps[head];
        if (sn.pending) { // both slots in flight: the oldest is this one
            HIPCHK(hipEventSynchronize(sn.done));
            sn.pending = false;
            tail = (head + 1) % 2;
        }
        const size_t bytes = elem * (size_t)cap;
        if (!sn.staged) {
            HIPCHK(hipEventCreateWithFlags(&sn.staged.e, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&sn.done.e, hipEventDisableTiming));
        }
        NRSCHK(sn.dPos.alloc(bytes));
        if (!sn.hPos) HIPCHK(hipHostMalloc(&sn.hPos.p, bytes, hipHostMallocDefault));
        if (withVel) {
            NRSCHK(sn.dVel.alloc(bytes));
            if (!sn.hVel) HIPCHK(hipHostMalloc(&sn.hVel.p, bytes, hipHostMallocDefault));
        }
        const size_t live = elem * (size_t)n;
        if (live) {
            HIPCHK(hipMemcpyAsync(sn.dPos.p, pos, live, hipMemcpyDeviceToDevice, stream));
            if (withVel) HIPCHK(hipMemcpyAsync(sn.dVel.p, vel, live, hipMemcpyDeviceToDevice, stream));
        }
        HIPCHK(hipEventRecord(sn.staged, stream));
        HIPCHK(hipStreamWaitEvent(copyStream, sn.staged, 0));
        if (live) {
            HIPCHK(hipMemcpyAsync(sn.hPos, sn.dPos.p, live, hipMemcpyDeviceToHost, copyStream));
            if (withVel) HIPCHK(hipMemcpyAsync(sn.hVel, sn.dVel.p, live, hipMemcpyDeviceToHost, copyStream));
        }
        HIPCHK(hipEventRecord(sn.done, copyStream));
        sn.n = n; sn.step = step; sn.withVel = withVel; sn.pending = true;
        head = (head + 1) % 2;
        return NRS_OK;
    }
    int wait(int block, const void **pos4, const void **vel4, uint64_t *np, uint64_t *step)
    {
        Snap &sn = snaps[tail];
        if (!sn.pending) return fail(NRS_E_STATE, "no snapshot in flight (nrs_snapshot_begin first)");
        if (block) {
            HIPCHK(hipEventSynchronize(sn.done));
        } else {
            const hipError_t e = hipEventQuery(sn.done);
            if (e == hipErrorNotReady) return NRS_E_NOTREADY;
            HIPCHK(e);
        }
        sn.pending = false;
        tail = (tail + 1) % 2;
        if (pos4) *pos4 = sn.hPos;
        if (vel4) *vel4 = sn.withVel ? (const void *)sn.hVel : nullptr;
        if (np) *np = sn.n;
        if (step) *step = sn.step;
        return NRS_OK;
    }
};

} // namespace nrs
