// nrs_boundary_tables.h — the boundary particles of a context and everything built from them: the host copies of the upload, the sorted
// (hash, index) pairs, the boundary cell table, the sorted particles, the near-boundary bit per cell, the kinematic bodies with their
// poses (nrs_host_bodies.h) and device arrays (nrs_kernels_bodies.h; DESIGN.md "Kinematic boundary bodies").  It depends on the
// precision alone; the context (nrs_ctx_impl.h) holds one, reads it through the views below and tells it, per call, the grid to build on
// (BoundaryGrid).  SPH::updateGpuBoundaries / updateGrid: sph/sph.cpp:313-337, 391-432.
//
// Two paths build the same tables.  At rest (set, new grid, bodies cleared while displaced): k_hash on a fresh upload, the sort,
// k_reorder_boundary; it allocates and synchronises.  Posed (the start of a step of a moving context): k_boundary_pose_hash on the
// resident rest positions, the sort, k_reorder_boundary_bodies; it allocates nothing, reads nothing back and is timed as
// NRS_STAGE_HASH.  What lies between the two kernels (sort_and_reset_cells) and after them (refresh_near_bits) is written once.
#pragma once
#include <functional>
#include <vector>

#include "nrs_ctx_base.h"
#include "nrs_host_bodies.h"
#include "nrs_host_profile.h"
#include "nrs_host_solver.h"
#include "nrs_kernels_ref.h"
#include "nrs_kernels_tiled.h"
#include "nrs_kernels_bodies.h"
#include "nrs_sort.h"

namespace nrs {

// the grid a rest build works on, as the context sees it at the time of the call
template <typename R> struct BoundaryGrid {
    const Params<R> &P;                 // the kernels' parameters (a slab rank: the grid of its cell-table window)
    unsigned sortBits;                  // sort_key_bits(P.numCells)
    bool wantNearBits;                  // the context runs list kernels on a power-of-two grid
    hipStream_t stream;
    std::function<int()> nearBitsReady; // called once the near bits are allocated, before they are filled (the context's wall list)
};

template <typename R> struct BoundaryTables {
    typedef typename Vec4T<R>::type T4;

    // ---- views ---------------------------------------------------------------------------------------------------------------------
    uint64_t count() const { return nb; }
    bool has_bodies() const { return bodies.n != 0; }
    bool near_bits_valid() const { return nearBitsValid; } // nearBits describes the current grid, and the context's wall list exists
    bool moving_step() const { return movingStep; }        // this step rebuilt the tables: DFSPH's A launches take the wall velocities
    uint32_t *cell_start() const { return bCellStart.as<uint32_t>(); }
    uint32_t *cell_end() const { return bCellEnd.as<uint32_t>(); }
    T4 *sorted() const { return bSorted.as<T4>(); }
    uint32_t *near_bits() const { return nearBits.as<uint32_t>(); }
    T4 *wall_velocities() const { return bdVel.as<T4>(); } // sorted order, of the posed build of this step
    // the boundary BufNames (nrs_host_solver.h): where the array lives and its bytes (per particle: in use; the cell tables: allocated);
    // false for any other name
    bool buffer(BufName b, void **p, size_t *bytes) const
    {
        switch (b) {
        case BUF_B_HASH_CUR: *p = bHashCur; *bytes = 4 * nb; return true;
        case BUF_B_INDEX_CUR: *p = bIndexCur; *bytes = 4 * nb; return true;
        case BUF_B_CELL_START: *p = bCellStart.p; *bytes = bCellStart.bytes; return true;
        case BUF_B_CELL_END: *p = bCellEnd.p; *bytes = bCellEnd.bytes; return true;
        case BUF_B_SORTED: *p = bSorted.p; *bytes = sizeof(T4) * nb; return true;
        case BUF_BD_BODY_SORTED: *p = bdBodySorted.p; *bytes = 4 * nb; return true;
        default: return false;
        }
    }

    // ---- the boundary half of the context's alloc_cells(): tables of C cells once there are particles; the ends start at zero -------
    int alloc_cells(uint64_t C)
    {
        if (!nb) return NRS_OK;
        NRSCHK(bCellStart.alloc(C * 4));
        NRSCHK(bCellEnd.alloc(C * 4));
        return NRS_OK;
    }
    int zero_cell_ends(uint64_t C, hipStream_t stream)
    {
        if (nb) HIPCHK(hipMemsetAsync(bCellEnd.p, 0, C * 4, stream));
        return NRS_OK;
    }

    // ---- nrs_set_boundaries: a new set of particles (it has no body assignment); the caller builds at rest next unless nb = 0 ---------
    void set_particles(const void *bi4, const void *vbi, uint64_t nbNew)
    {
        nb = nbNew;
        clear_bodies();
        hostBi.assign((const T4 *)bi4, (const T4 *)bi4 + nb);
        hostVbi.assign((const R *)vbi, (const R *)vbi + nb);
        if (!nb) nearBitsValid = false;
    }

    // The tables at the uploaded positions.  The cell tables are allocated for g.P.numCells (the context's alloc_cells()).
    int build_at_rest(const BoundaryGrid<R> &g)
    {
        if (!nb) return NRS_OK;
        if ((size_t)g.P.numCells * 4 > bCellStart.bytes) return fail(NRS_E_STATE, "boundary tables: the cell tables are smaller than the grid");
        const hipStream_t stream = g.stream;
        DevBuf dBi, dVbi;
        NRSCHK(dBi.alloc(sizeof(T4) * nb));
        NRSCHK(dVbi.alloc(sizeof(R) * nb));
        HIPCHK(hipMemcpyAsync(dBi.p, hostBi.data(), sizeof(T4) * nb, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dVbi.p, hostVbi.data(), sizeof(R) * nb, hipMemcpyHostToDevice, stream));
        NRSCHK(bHash.alloc(4 * nb)); NRSCHK(bIndex.alloc(4 * nb)); NRSCHK(bHashAlt.alloc(4 * nb)); NRSCHK(bIndexAlt.alloc(4 * nb));
        NRSCHK(bSorted.alloc(sizeof(T4) * nb));
        hipLaunchKernelGGL((k_hash<R>), dim3(nblocks(nb)), dim3(BLOCK), 0, stream, g.P, dBi.as<T4>(), bHash.as<uint32_t>(),
                           bIndex.as<uint32_t>(), (uint32_t)nb);
        const size_t tmp = sort_bytes(g.sortBits, stream);
        if (!tmp) return fail(NRS_E_HIP, NO_SORT_SIZE);
        DevBuf t;
        NRSCHK(t.alloc(tmp));
        NRSCHK(sort_and_reset_cells(g.P, g.sortBits, t.p, tmp, stream));
        hipLaunchKernelGGL((k_reorder_boundary<R>), dim3(nblocks(nb)), dim3(BLOCK), 0, stream, bHashCur, bIndexCur,
                           dBi.as<T4>(), dVbi.as<R>(), bSorted.as<T4>(), bCellStart.as<uint32_t>(),
                           bCellEnd.as<uint32_t>(), (uint32_t)nb);
        nearBitsValid = false;
        if (g.wantNearBits) {
            NRSCHK(nearBits.alloc(near_bytes(g.P)));
            NRSCHK(g.nearBitsReady());
            NRSCHK(refresh_near_bits(g.P, stream));
            nearBitsValid = true;
        }
        if (bodies.n) { // the tables above hold the REST poses: sorted ids for them, and a rebuild at the poses before the next step
            NRSCHK(bodies_at_rest(stream));
            bodies.dirty = bodies.displaced();
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        return NRS_OK;
    }

    // ---- kinematic boundary bodies ---------------------------------------------------------------------------------------------------
    // The poses live in `bodies` (host, double); only while it is moving does a step touch the boundary tables.
    // nrs_set_boundary_bodies after the context's own refusals; slab: the context has a slab decomposition
    int set_bodies(const uint32_t *bodyOf, uint64_t nbGiven, uint32_t nbodies, bool slab, const BoundaryGrid<R> &g)
    {
        if (!nb) return fail(NRS_E_STATE, "nrs_set_boundary_bodies before nrs_set_boundaries");
        if (!bodyOf || nbodies <= 1) return clear_bodies_to_rest(g); // clear: the walls return to the uploaded positions
        if (slab) return fail(NRS_E_INVALID, "slab contexts have no boundary bodies");
        if (nbGiven != nb) return fail(NRS_E_INVALID, "nb differs from the context's boundary particle count");
        if (nbodies > (uint32_t)NRS_MAX_BODIES) return fail(NRS_E_INVALID, "more than NRS_MAX_BODIES bodies");
        double sum[NRS_MAX_BODIES][3] = {{0.0}};
        uint64_t cnt[NRS_MAX_BODIES] = {0};
        for (uint64_t i = 0; i < nb; ++i) {
            const uint32_t k = bodyOf[i];
            if (k >= nbodies) return fail(NRS_E_INVALID, "body id >= nbodies");
            sum[k][0] += (double)hostBi[i].x; sum[k][1] += (double)hostBi[i].y; sum[k][2] += (double)hostBi[i].z;
            ++cnt[k];
        }
        NRSCHK(clear_bodies_to_rest(g)); // (a new assignment starts from the rest poses)
        const hipStream_t stream = g.stream;
        NRSCHK(bdRest.alloc(sizeof(T4) * nb)); NRSCHK(bdVbi.alloc(sizeof(R) * nb)); NRSCHK(bdBodyOf.alloc(4 * nb));
        NRSCHK(bdWorld.alloc(sizeof(T4) * nb)); NRSCHK(bdBodySorted.alloc(4 * nb)); NRSCHK(bdVel.alloc(sizeof(T4) * nb));
        const size_t tmp = std::max(sort_bytes(g.sortBits, stream), sort_bytes(32u, stream));
        if (!tmp) return fail(NRS_E_HIP, NO_SORT_SIZE);
        NRSCHK(bdSortTmp.alloc(tmp));
        HIPCHK(hipMemcpyAsync(bdRest.p, hostBi.data(), sizeof(T4) * nb, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(bdVbi.p, hostVbi.data(), sizeof(R) * nb, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(bdBodyOf.p, bodyOf, 4 * nb, hipMemcpyHostToDevice, stream));
        NRSCHK(bodies_at_rest(stream));
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream)); // the caller may reuse body_of on return
        bodies.init(nbodies, sum, cnt);
        return NRS_OK;
    }
    int set_body_velocity(uint32_t body, const double *v, const double *omega) { return bodies.set_velocity(body, v, omega); }
    int set_body_pose(uint32_t body, const double *x, const double *q) { return bodies.set_pose(body, x, q); }
    int get_body_pose(uint32_t body, double *x, double *q) const { return bodies.get_pose(body, x, q); }

    // Start of a step of a moving context: advance the poses by dt (host, double), round the table to SReal, rebuild the tables on the
    // stream.  No synchronisation, no allocation, no read-back.  Timed as NRS_STAGE_HASH.
    int advance_and_rebuild(const Params<R> &P, double dt, unsigned sortBits, StageTimer &timer, uint32_t profMask, hipStream_t stream)
    {
        movingStep = bodies.moving();
        if (!movingStep) return NRS_OK;
        bodies.advance(dt);
        BodyTable<R> T;
        std::memset(&T, 0, sizeof(T));
        for (uint32_t k = 1; k < bodies.n; ++k) {
            const BodyPoses::Body &b = bodies.b[k];
            double rot[9];
            bodies.rotation(k, rot);
            BodyPose<R> &o = T.b[k];
            for (int a = 0; a < 9; ++a) o.rot[a] = (R)rot[a];
            for (int a = 0; a < 3; ++a) { o.x[a] = (R)b.x[a]; o.c[a] = (R)b.c[a]; o.v[a] = (R)b.v[a]; o.w[a] = (R)b.w[a]; }
        }
        const uint32_t NB = (uint32_t)nb;
        if (sort_bytes(sortBits, stream) > bdSortTmp.bytes || (size_t)P.numCells * 4 > bCellStart.bytes)
            return fail(NRS_E_STATE, "boundary bodies: the grid outgrew the storage sized at nrs_set_boundary_bodies (assign the bodies again)");
        NRSCHK(timer.begin(NRS_STAGE_HASH, false, profMask, stream));
        hipLaunchKernelGGL((k_boundary_pose_hash<R>), dim3(nblocks(NB)), dim3(BLOCK), 0, stream, P, T, bdRest.as<T4>(), bdVbi.as<R>(),
                           bdBodyOf.as<uint32_t>(), bdWorld.as<T4>(), bHash.as<uint32_t>(), bIndex.as<uint32_t>(), NB);
        NRSCHK(sort_and_reset_cells(P, sortBits, bdSortTmp.p, bdSortTmp.bytes, stream));
        hipLaunchKernelGGL((k_reorder_boundary_bodies<R>), dim3(nblocks(NB)), dim3(BLOCK), 0, stream, bHashCur, bIndexCur, T, bdWorld.as<T4>(),
                           bdBodyOf.as<uint32_t>(), bSorted.as<T4>(), bdBodySorted.as<uint32_t>(), bdVel.as<T4>(), bCellStart.as<uint32_t>(),
                           bCellEnd.as<uint32_t>(), NB);
        if (nearBitsValid) NRSCHK(refresh_near_bits(P, stream));
        HIPCHK(hipGetLastError());
        NRSCHK(timer.end(stream));
        bodies.dirty = false;
        return NRS_OK;
    }

private:
    static constexpr const char *NO_SORT_SIZE = "rocprim::radix_sort_pairs: no temporary storage size for the boundary sort";
    uint64_t nb = 0;
    std::vector<T4> hostBi; // the upload, kept: every rest build starts from it
    std::vector<R> hostVbi;
    DevBuf bSorted, bHash, bIndex, bHashAlt, bIndexAlt;
    uint32_t *bHashCur = nullptr, *bIndexCur = nullptr; // the sorted pairs: whichever of each pair the last sort left them in
    DevBuf bCellStart, bCellEnd;
    DevBuf nearBits; // nrs_kernels_tiled.h: one bit per cell, set within one cell of a boundary particle
    bool nearBitsValid = false;
    BodyPoses bodies;
    bool movingStep = false;
    DevBuf bdRest, bdVbi, bdBodyOf, bdWorld, bdBodySorted, bdVel, bdSortTmp;

    void clear_bodies() { bodies.clear(); movingStep = false; }
    // no assignment any more; tables that stood at displaced poses (or were about to) are rebuilt at rest
    int clear_bodies_to_rest(const BoundaryGrid<R> &g)
    {
        const bool displaced = bodies.n && (bodies.displaced() || bodies.dirty);
        clear_bodies();
        if (displaced) NRSCHK(build_at_rest(g));
        return NRS_OK;
    }
    // the sorted body ids of tables at rest, and walls that stand still
    int bodies_at_rest(hipStream_t stream)
    {
        hipLaunchKernelGGL(k_gather_body, dim3(nblocks(nb)), dim3(BLOCK), 0, stream, bIndexCur, bdBodyOf.as<uint32_t>(), bdBodySorted.as<uint32_t>(),
                           (uint32_t)nb);
        HIPCHK(hipMemsetAsync(bdVel.p, 0, sizeof(T4) * nb, stream));
        return NRS_OK;
    }
    PairBuffers pairs() const { return PairBuffers{bHash.as<uint32_t>(), bHashAlt.as<uint32_t>(), bIndex.as<uint32_t>(), bIndexAlt.as<uint32_t>()}; }
    // temporary storage of the sort below (sort_pairs_plain, nrs_sort.h); 0: the sort gave none
    size_t sort_bytes(unsigned bits, hipStream_t stream) const
    {
        size_t tmp = 0;
        PairBuffers p = pairs();
        if (sort_pairs_plain(nullptr, tmp, p, (size_t)nb, bits, stream) != hipSuccess) return 0;
        return tmp;
    }
    // the middle of both builds: the pairs a front kernel left in bHash / bIndex sorted by hash, and an empty cell table for the reorder
    // kernel to fill
    int sort_and_reset_cells(const Params<R> &P, unsigned bits, void *tmp, size_t tmpBytes, hipStream_t stream)
    {
        PairBuffers p = pairs();
        HIPCHK(sort_pairs_plain(tmp, tmpBytes, p, (size_t)nb, bits, stream));
        bHashCur = p.key;
        bIndexCur = p.val;
        HIPCHK(hipMemsetAsync(bCellStart.p, 0xff, (size_t)P.numCells * 4, stream));
        return NRS_OK;
    }
    static size_t near_bytes(const Params<R> &P) { return (((size_t)P.numCells + 31) / 32) * 4; }
    int refresh_near_bits(const Params<R> &P, hipStream_t stream)
    {
        HIPCHK(hipMemsetAsync(nearBits.p, 0, near_bytes(P), stream));
        hipLaunchKernelGGL((k_mark_near_boundary<R>), dim3(nblocks(nb)), dim3(BLOCK), 0, stream, P, bHashCur, (uint32_t)nb, nearBits.as<uint32_t>());
        return NRS_OK;
    }
};

} // namespace nrs
