// nrs_diffuse.h — the owner of everything the diffuse particles keep on the device (DESIGN.md "Diffuse particles"): the header with
// the counters, the living set (positions with lifetimes, velocities, kinds), its staging copy and survivor flags, the workgroup totals of
// the two scans, and the per-fluid arrays of the last step (density gradients, potentials, births, parents' kinds).  Nothing is allocated
// before the first step or upload; nrs_diffuse_release frees everything.  It stands beside the FieldSampler (nrs_field_sampler.h): the
// holder of both (nrs_readers.h) refuses what has to be refused, has the sampler build its particle grid and hands its views to step().  The
// host decisions — what is accepted, sizes, which result an id means, the per-particle rules — are in nrs_host_diffuse.h.
#pragma once
#include "nrs_ctx_base.h"
#include "nrs_host_diffuse.h"
#include "nrs_kernels_diffuse.h"

namespace nrs {

struct DiffuseSystem {
    nrs_diffuse_config cfg = {};
    DiffuseLast last;
    uint64_t steps = 0; // diffuse steps since configure: the hash's step word

    // nrs_diffuse_configure (cfg is checked): no allocation, no launch; the header is brought up to date by the next call that uses it
    void configure(const nrs_diffuse_config &c)
    {
        if (last.configured && c.capacity != cfg.capacity) pendEmpty = true; // another capacity: the living set goes
        cfg = c;
        last.configured = true;
        last.stepped = false;
        steps = 0;
        pendClear = true;
    }

    void *result(uint32_t which) const
    {
        switch (which) {
        case NRS_DIFFUSE_POS: return pos.p;
        case NRS_DIFFUSE_VEL: return vel.p;
        case NRS_DIFFUSE_KIND: return kind.p;
        case NRS_DIFFUSE_POTENTIALS: return potentials.p;
        case NRS_DIFFUSE_BIRTHS: return births.p;
        case NRS_DIFFUSE_NORMALS: return normals.p;
        default: return nullptr;
        }
    }

    // the living count, waited for
    int alive_now(hipStream_t stream, uint64_t *alive)
    {
        *alive = 0;
        if (!hdr.p) return NRS_OK;
        NRSCHK(flush(stream));
        uint32_t a = 0;
        HIPCHK(hipMemcpyAsync(&a, hdr.p, 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        *alive = a;
        return NRS_OK;
    }
    // nrs_diffuse_count: waits
    int count(hipStream_t stream, uint64_t *alive, uint64_t byKind[3], uint64_t *dropped)
    {
        DiffuseHeader h = {};
        if (hdr.p) {
            NRSCHK(flush(stream));
            hipLaunchKernelGGL(k_diffuse_kinds, dim3(1), dim3(SCAN_BLOCK), 0, stream, (const uint32_t *)kind.as<uint32_t>(), hdr.as<DiffuseHeader>());
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&h, hdr.p, sizeof(h), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
        }
        if (alive) *alive = h.alive;
        if (byKind) for (int a = 0; a < 3; ++a) byKind[a] = h.byKind[a];
        if (dropped) *dropped = pendClear ? 0 : h.dropped;
        return NRS_OK;
    }

    // nrs_diffuse_upload (checked): replaces the living set; waits
    template <typename R> int upload(const void *pos4, const void *vel4, uint64_t n, hipStream_t stream)
    {
        typedef typename Vec4T<R>::type T4;
        NRSCHK(ensure_set<R>(stream));
        if (n) {
            HIPCHK(hipMemcpyAsync(pos.p, pos4, sizeof(T4) * n, hipMemcpyHostToDevice, stream));
            HIPCHK(hipMemcpyAsync(vel.p, vel4, sizeof(T4) * n, hipMemcpyHostToDevice, stream));
            HIPCHK(hipMemsetAsync(kind.p, 0, 4 * n, stream));
        }
        hipLaunchKernelGGL(k_diffuse_header, dim3(1), dim3(1), 0, stream, hdr.as<DiffuseHeader>(), (uint32_t)n, 1, 0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        return NRS_OK;
    }

    // One diffuse step over the N sorted fluid particles sP / sV of the sampler's grid G (its cell table, nSorted = N, err).  Enqueues on
    // `stream`; waits for nothing unless a buffer has to grow.
    template <typename R, int KSET>
    int step(const Params<R> &P, const GridView<R> &G, const typename Vec4T<R>::type *sP, const typename Vec4T<R>::type *sV, uint32_t N, R dt,
             hipStream_t stream)
    {
        typedef typename Vec4T<R>::type T4;
        NRSCHK(ensure_set<R>(stream));
        const uint32_t cap = cfg.capacity, nbD = nblocks(cap), nbF = nblocks(N);
        const DiffuseCfg<R> C = diffuse_cfg<R>(cfg);
        DiffuseHeader *H = hdr.as<DiffuseHeader>();
        const DiffuseSet<R> cur{pos.as<T4>(), vel.as<T4>(), kind.as<uint32_t>()}, staged{posT.as<T4>(), velT.as<T4>(), kindT.as<uint32_t>()};
        if (N) {
            NRSCHK(normals.alloc(sizeof(T4) * (size_t)N)); NRSCHK(potentials.alloc(sizeof(T4) * (size_t)N));
            NRSCHK(births.alloc(4 * (size_t)N)); NRSCHK(parentKind.alloc(4 * (size_t)N)); NRSCHK(birthTot.alloc(4 * (size_t)nbF));
            const SampleOut<R> O{nullptr, normals.as<T4>(), nullptr, nullptr};
            hipLaunchKernelGGL((k_sample_points<R, KSET, false>), dim3(nbF), dim3(BLOCK), 0, stream, P, G, sP, sV, sP, Lattice(), O,
                               (uint32_t)NRS_FIELD_GRADIENT, N);
            const DiffuseFluidOut<R> F{potentials.as<T4>(), births.as<uint32_t>(), parentKind.as<uint32_t>(), birthTot.as<uint32_t>()};
            hipLaunchKernelGGL((k_diffuse_potentials<R, KSET>), dim3(nbF), dim3(BLOCK), 0, stream, P, G, sP, sV, (const T4 *)normals.as<T4>(), C, steps, dt, F, N);
        }
        hipLaunchKernelGGL((k_diffuse_advect<R, KSET>), dim3(nbD), dim3(BLOCK), 0, stream, P, G, sP, sV, C, dt, (const DiffuseHeader *)H, cur, staged,
                           flag.as<uint32_t>(), keepTot.as<uint32_t>());
        hipLaunchKernelGGL(k_diffuse_scan, dim3(1), dim3(SCAN_BLOCK), 0, stream, keepTot.as<uint32_t>(), nbD, birthTot.as<uint32_t>(), N ? nbF : 0u, cap, H);
        hipLaunchKernelGGL((k_diffuse_compact<R>), dim3(nbD), dim3(BLOCK), 0, stream, (const uint32_t *)flag.as<uint32_t>(),
                           (const uint32_t *)keepTot.as<uint32_t>(), staged, cur, cap);
        if (N)
            hipLaunchKernelGGL((k_diffuse_births<R>), dim3(nbF), dim3(BLOCK), 0, stream, P, sP, sV, C, steps, dt, (const uint32_t *)births.as<uint32_t>(),
                               (const uint32_t *)parentKind.as<uint32_t>(), (const uint32_t *)birthTot.as<uint32_t>(), (const DiffuseHeader *)H, cur, N);
        HIPCHK(hipGetLastError());
        ++steps;
        last.stepped = true;
        last.N = N;
        return NRS_OK;
    }

    // nrs_diffuse_release: every buffer goes (the caller has drained the stream); the configuration stays, the set is empty
    void release()
    {
        for (DevBuf *b : {&hdr, &pos, &vel, &kind, &posT, &velT, &kindT, &flag, &keepTot, &birthTot, &normals, &potentials, &births, &parentKind}) b->release();
        allocCap = 0;
        pendEmpty = false;
        last.stepped = false;
        last.N = 0;
    }

private:
    // the header and the arrays sized by the capacity; the header's pending changes
    template <typename R> int ensure_set(hipStream_t stream)
    {
        typedef typename Vec4T<R>::type T4;
        if (!hdr.p) {
            NRSCHK(hdr.alloc(sizeof(DiffuseHeader)));
            HIPCHK(hipMemsetAsync(hdr.p, 0, sizeof(DiffuseHeader), stream));
            pendEmpty = pendClear = false;
        }
        const size_t cap = cfg.capacity;
        if (allocCap != cfg.capacity) {
            if (allocCap) {
                HIPCHK(hipStreamSynchronize(stream)); // queued launches may still use the arrays of the old capacity
                for (DevBuf *b : {&pos, &vel, &kind, &posT, &velT, &kindT, &flag, &keepTot}) b->release();
                pendEmpty = true;
            }
            NRSCHK(pos.alloc(sizeof(T4) * cap)); NRSCHK(vel.alloc(sizeof(T4) * cap)); NRSCHK(kind.alloc(4 * cap));
            NRSCHK(posT.alloc(sizeof(T4) * cap)); NRSCHK(velT.alloc(sizeof(T4) * cap)); NRSCHK(kindT.alloc(4 * cap));
            NRSCHK(flag.alloc(4 * cap)); NRSCHK(keepTot.alloc(4 * (size_t)nblocks(cap)));
            allocCap = cfg.capacity;
        }
        return flush(stream);
    }
    int flush(hipStream_t stream)
    {
        if (!hdr.p || !(pendEmpty || pendClear)) return NRS_OK;
        hipLaunchKernelGGL(k_diffuse_header, dim3(1), dim3(1), 0, stream, hdr.as<DiffuseHeader>(), 0u, pendEmpty ? 1 : 0, pendClear ? 1 : 0);
        HIPCHK(hipGetLastError());
        pendEmpty = pendClear = false;
        return NRS_OK;
    }

    DevBuf hdr;                                    // DiffuseHeader
    DevBuf pos, vel, kind;                         // the living set: SVec4[capacity] x 2, uint32[capacity]
    DevBuf posT, velT, kindT, flag;                // the advected state of a step before compaction, and who survives
    DevBuf keepTot, birthTot;                      // survivors / births per workgroup, scanned in place
    DevBuf normals, potentials, births, parentKind; // per sorted fluid particle of the last step
    uint32_t allocCap = 0;                         // capacity the set's arrays were allocated for (0: none)
    bool pendEmpty = false, pendClear = false;     // the header still has to: empty the set, restart `dropped`
};

} // namespace nrs
