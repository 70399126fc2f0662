// nrs_inflow.h — the owner of what the sources and sinks keep (DESIGN.md "Sources and sinks"): the emitter slots with their
// accumulators and counts, the sink configuration and its counts on the host; on the device the workgroup totals of the cull, its
// header, and the row tables of disc emitters.  Nothing is allocated before the first cull or the first emission of a disc.  Unlike
// the add-ons that only read the particles (nrs_readers.h) it is the context's own member: the context (nrs_ctx_impl.h) refuses what has
// to be refused, hands over its arrays and applies what a call reports (the new count, the pointer swap, the state transition).  The host decisions are nrs_host_inflow.h's.
#pragma once
#include "nrs_ctx_base.h"
#include "nrs_host_inflow.h"
#include "nrs_kernels_inflow.h"

namespace nrs {

struct InflowSystem {
    EmitterSlot slots[NRS_MAX_EMITTERS];
    bool haveSinks = false;
    nrs_sink_config sinks = {};
    uint64_t removedTotal = 0, culls = 0, stepsSeen = 0; // since nrs_sinks_set

    uint32_t emitters_used() const
    {
        uint32_t c = 0;
        for (const EmitterSlot &s : slots) c += s.used ? 1u : 0u;
        return c;
    }
    bool emitter_enabled() const
    {
        for (const EmitterSlot &s : slots)
            if (s.used && s.e.enabled) return true;
        return false;
    }
    bool configured() const { return haveSinks || emitters_used() != 0; }
    bool active() const { return haveSinks || emitter_enabled(); } // a step has something to do at its top

    void set_sinks(const nrs_sink_config *c)
    {
        haveSinks = c != nullptr;
        if (c) sinks = *c; else std::memset(&sinks, 0, sizeof(sinks));
        removedTotal = culls = stepsSeen = 0;
    }
    // the step about to run counts; true: it culls first
    bool cull_due()
    {
        if (!haveSinks) return false;
        ++stepsSeen;
        return inflow_cull_due(stepsSeen, sinks.interval);
    }

    // the step cull_due() counted was refused before anything moved (particle ids exhausted, nrs_track.h)
    void step_not_taken() { if (haveSinks) --stepsSeen; }

    // Count the survivors among the n particles at pos (B: the bounds), wait, and report them.  Nothing is moved.
    template <typename R> int count(const typename Vec4T<R>::type *pos, const CullBounds<R> &B, uint32_t n, hipStream_t stream, uint32_t *survivors)
    {
        const uint32_t nb = nblocks(n);
        NRSCHK(blockTot.alloc(4 * (size_t)nb));
        NRSCHK(hdr.alloc(sizeof(InflowHeader)));
        hipLaunchKernelGGL((k_cull_count<R>), dim3(nb), dim3(BLOCK), 0, stream, pos, B, n, blockTot.as<uint32_t>());
        hipLaunchKernelGGL(k_cull_scan, dim3(1), dim3(SCAN_BLOCK), 0, stream, blockTot.as<uint32_t>(), nb, hdr.as<InflowHeader>());
        HIPCHK(hipGetLastError());
        InflowHeader h = {};
        HIPCHK(hipMemcpyAsync(&h, hdr.p, sizeof(h), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        *survivors = h.survivors;
        return NRS_OK;
    }
    // the survivors of the last count() to the front of the target arrays, in order (same pos, B and n)
    template <typename R> int compact(const CullArrays<R> &A, const CullBounds<R> &B, uint32_t n, hipStream_t stream)
    {
        hipLaunchKernelGGL((k_cull_compact<R>), dim3(nblocks(n)), dim3(BLOCK), 0, stream, A, B, n, (const uint32_t *)blockTot.as<uint32_t>());
        HIPCHK(hipGetLastError());
        return NRS_OK;
    }
    void culled(uint64_t removed) { ++culls; removedTotal += removed; }

    // the layers of slot `si` at the given offsets (inflow_schedule) behind O.first; enqueues
    template <typename R> int emit(uint32_t si, const std::vector<double> &offsets, EmitOut<R> O, hipStream_t stream)
    {
        EmitterSlot &sl = slots[si];
        const bool disc = sl.e.shape == NRS_EMITTER_DISC;
        if (disc && sl.tableDirty) {
            const size_t rows = sl.sites.half.size();
            NRSCHK(rowHalf[si].alloc(4 * rows));
            NRSCHK(rowStart[si].alloc(4 * rows));
            HIPCHK(hipMemcpyAsync(rowHalf[si].p, sl.sites.half.data(), 4 * rows, hipMemcpyHostToDevice, stream));
            HIPCHK(hipMemcpyAsync(rowStart[si].p, sl.sites.start.data(), 4 * rows, hipMemcpyHostToDevice, stream));
            HIPCHK(hipStreamSynchronize(stream)); // once per nrs_emitter_set of a disc: the slot's host arrays may go with the next set
            sl.tableDirty = false;
        }
        EmitArgs A;
        std::memset(&A, 0, sizeof(A));
        for (int a = 0; a < 3; ++a) { A.e1[a] = sl.f.e1[a]; A.e2[a] = sl.f.e2[a]; A.v[a] = sl.e.speed * sl.f.d[a]; }
        A.s = sl.s;
        A.sites = (uint32_t)sl.sites.sites; A.ku = sl.sites.ku; A.kv = sl.sites.kv; A.disc = disc ? 1u : 0u;
        for (size_t l0 = 0; l0 < offsets.size(); l0 += INFLOW_LAYERS_PER_LAUNCH) {
            A.layers = (uint32_t)std::min<size_t>(INFLOW_LAYERS_PER_LAUNCH, offsets.size() - l0);
            for (uint32_t l = 0; l < A.layers; ++l) inflow_origin(sl, offsets[l0 + l], A.o[l]);
            hipLaunchKernelGGL((k_inflow_emit<R>), dim3(nblocks((uint64_t)A.layers * A.sites)), dim3(BLOCK), 0, stream, A,
                               (const int32_t *)rowHalf[si].as<int32_t>(), (const uint32_t *)rowStart[si].as<uint32_t>(), O);
            O.first += A.layers * A.sites;
            O.firstId += A.layers * A.sites;
        }
        HIPCHK(hipGetLastError());
        return NRS_OK;
    }
    // nrs_emit_block: the m nodes of L behind O.first; enqueues
    template <typename R> int emit_block(const Lattice &L, const double vel[3], uint32_t m, EmitOut<R> O, hipStream_t stream)
    {
        hipLaunchKernelGGL((k_inflow_block<R>), dim3(nblocks(m)), dim3(BLOCK), 0, stream, L, vel[0], vel[1], vel[2], m, O);
        HIPCHK(hipGetLastError());
        return NRS_OK;
    }
    // nrs_emit_mesh: the m selected nodes sel[0 .. m) of L (device, linear indices) behind O.first; enqueues
    template <typename R> int emit_sites(const Lattice &L, const uint32_t *sel, const double vel[3], uint32_t m, EmitOut<R> O, hipStream_t stream)
    {
        if (!m) return NRS_OK;
        hipLaunchKernelGGL((k_inflow_sites<R>), dim3(nblocks(m)), dim3(BLOCK), 0, stream, L, sel, vel[0], vel[1], vel[2], m, O);
        HIPCHK(hipGetLastError());
        return NRS_OK;
    }

private:
    DevBuf blockTot, hdr;                                     // survivors per workgroup, scanned in place; InflowHeader
    DevBuf rowHalf[NRS_MAX_EMITTERS], rowStart[NRS_MAX_EMITTERS]; // disc emitters: InflowSites::half / start
};

} // namespace nrs
