// nrs_ctx_impl.h — the context object behind the C ABI of libnereus_hip.so (include/nereus_hip.h; entry points in nrs_abi.hip).
//
// The context owns the device-resident particle state and sequences one update() exactly as the
// reference's host classes do (SPH::update sph/sph.cpp:215-285, IISPH::update sph/iisph/iisph.cpp:170-217,
// predictAdvection/pressureSolve sph/sph_cuda.cu:513-899) — minus the per-step PCIe copies: the
// "unsorted" arrays of step t+1 are the integrated sorted arrays of step t (buffer swap), which is what
// the reference obtains by copying sorted→host→device.
//
// Ctx<R, KSET, SURF> keeps the particle arrays, the cell table and the hit lists, the hash and reorder launches of the sort stage, the
// SESPH tail, and what frames every step: the step plan, the last launch that leaves the next step's keys, the end of the step.
// Everything else has one owner outside it, held as one member, read through views and driven through named operations; no buffer of
// theirs is assigned here.  The pressure solvers — IISPH, PCISPH, PBF, DFSPH, with Akinci's surface model — are one of them: ps
// (PressureSolvers<R, KSET, SURF>, nrs_solvers.h) has their buffers, settings, derived constants and statistics and launches their
// chains; the context tells it per chain what the step is now (solver_step) and lends it launch_last.  The reductions both use are
// red's (Reductions<R>, nrs_solvers.h).
// The boundary particles, their tables and bodies depend on the precision alone: bt (BoundaryTables<R>, nrs_boundary_tables.h), which
// launches its own builds.  So does the slab exchange: exch (SlabExchange<R>, nrs_slab_exchange.h) has the cuts, the window, the last
// pack, the ghost streams, block counts, totals and flags of the partition, the pinned landing and the pack's event, and launches the
// slab kernels; the context decides the refusals and applies what a pack or unpack means to n, nOwned and the array state.  The
// step's wall list, sized by the fluid, is templated on nothing: wlist (WallLists, nrs_wall_list.h).  Nor is the sort stage's state:
// sort (SortStage, nrs_sort.h; compiled once, in nrs_sort.hip, with the radix sorts and the merge) has the (hash, index) pairs and
// which of each is current, prepared or a pack target, the sort's workspace, the buffers of the coherent re-sort, its mover-count
// word and statistics.  The context reads views of it (sort.hash(), sort.index(), sort.prepared(), the tile counts the fused and the
// slab kernels write) and calls its operations (sort_keys, scan_movers, split, scan_holes, the pack targets).  The add-ons that only
// read the particle state — field sampling, surface extraction, diffuse particles — depend on the precision and the kernel set: rd
// (FluidReaders<R, KSET>, nrs_readers.h) holds their buffers, launches on them and copies their results out; the context tells it per call
// what the fluid is now (fluid_now).  The sources and sinks change n and the array state: their buffers are inflow's (InflowSystem, nrs_inflow.h).
// Particle tracking follows the particle arrays — gathered where they are reordered, swapped where they swap, written where particles are
// created: the ids, births and records, the id counter and the emit values are track's (TrackSystem, nrs_track.h).
// Host bookkeeping that depends on none of them lives in plain structs the context holds as members, or in pure functions it calls:
// the stage timer (nrs_host_profile.h), the snapshot ring (nrs_host_snapshot.h), the solver settings and their validation
// (nrs_host_settings.h), the grid a boundary box asks for (nrs_host_grid.h), the decisions of the slab exchange — window, partition
// form, stream totals, unpack offsets — (nrs_host_slab.h), the state of the particle arrays with its transitions and the sort stage's
// choice (nrs_host_state.h), the step plan and the exit rule of the solver loops (nrs_host_plan.h), what differs by solver — stages,
// stale and derived constants, buffers, what an array or statistic id means — with one state struct per solver (nrs_host_solver.h),
// the geometry of the neighbour scan — the cell-table window that makes P of PU, the cut-offs of the exact test, the quantisation
// set-up of the compact scan, the wall workgroups of a launch — (nrs_host_scan.h, which the kernels include too: nrs_math.h).
// Every buffer, pinned landing and event frees itself (DevBuf, PinnedBuf, Event: nrs_ctx_base.h); ~Ctx only synchronises.
#pragma once
#include "nrs_ctx_base.h"
#include "nrs_boundary_tables.h"
#include "nrs_host_grid.h"
#include "nrs_host_plan.h"
#include "nrs_host_profile.h"
#include "nrs_host_settings.h"
#include "nrs_host_slab.h"
#include "nrs_host_snapshot.h"
#include "nrs_host_solver.h"
#include "nrs_host_state.h"
#include "nrs_sort.h"
#include "nrs_wall_list.h"

#include "nrs_kernels_ref.h"
#include "nrs_kernels_tiled.h"
#include "nrs_kernels_staged.h"
#include <type_traits>
#include "nrs_solvers.h"
#include "nrs_kernels_bodies.h"
#include "nrs_slab_exchange.h"
#include "nrs_readers.h"
#include "nrs_inflow.h"
#include "nrs_mesh.h"
#include "nrs_track.h"
#include "nrs_kernels_resort.h"
#include <climits>

namespace nrs {

template <typename R, int KSET, bool SURF> struct Ctx : CtxBase {
    typedef typename Vec4T<R>::type T4;
    // PU: the parameters as the caller set them (GLOBAL grid; what nrs_get_params returns).  P: what the kernels get — PU
    // with numBodies = first column of the cell-table window (0 = whole grid) and, for a slab rank, gridSize[0] / numCells of
    // that window: a rank keeps cell tables only for its own cell-x columns + halo, so table memory (and the radix-sort key
    // width) stop growing with the number of ranks.  Cell coordinates stay global (calcGridPos is unchanged), only the hash
    // rebases x: the sort order, and with it every per-particle result, is the one of the global grid.
    Params<R> PU, P;
    SlabExchange<R> exch; // the cuts, the window, the last pack and its totals, the exchange's buffers and launches (nrs_slab_exchange.h)
    // geo: the scan's geometry for P — the quantisation set-up of the compact scan (and whether the grid allows it) and the two
    // cut-offs of the exact test (nrs_host_scan.h).  Both follow P: derived here, wherever the parameters or the window change.
    ScanGeometry geo{};
    void derive_kernel_params()
    {
        P = window_params(PU, exch.host().winW, exch.host().winBase);
        geo = scan_geometry(P);
    }
    DevBuf gatherPos; // (x, y, z, p / rho^2), (vx, vy, vz, m / rho) side by side per sorted slot: density kernel -> force kernel of the same step (HitBuffer)
    DevBuf qpos; // one word per sorted slot (+ 4 slots of padding), written by the reorder kernels
    nrs_config cfg;
    uint64_t cap = 0, n = 0;
    bool midStep = false; // a partial step left the state mid-update
    // particle state: A = current ("unsorted" input of the next step), B = sorted work arrays
    DevBuf posA, posB, velA, velB, presA, presB, dens, forces;
    SortStage sort; // the (hash, index) pairs, the sort's workspace, the coherent re-sort and its statistics (nrs_sort.h)
    DevBuf cellStart, cellEnd;
    uint32_t cellsAllocated = 0;
    BoundaryTables<R> bt; // the boundary particles, their tables and bodies (nrs_boundary_tables.h)
    Reductions<R> red;    // sums, maxima and the hit statistics (nrs_solvers.h)
    ViscositySolver<R> visc; // DFSPH's implicit viscosity solve: settings, buffers, the CG loop (nrs_viscosity.h)
    PressureSolvers<R, KSET, SURF> ps{red, visc}; // IISPH, PCISPH, PBF, DFSPH, Akinci: buffers, settings, chains (nrs_solvers.h)
    // where a buffer of the given name lives: the boundary's are bt's, the solvers' ps's (whose switch has no default: -Wswitch names a
    // BufName nobody answers for), the sorted keys / values are pointers into a pair
    void *buf_ptr(BufName b)
    {
        void *p = nullptr;
        size_t bytes = 0;
        if (bt.buffer(b, &p, &bytes) || ps.buffer(b, &p, &bytes)) return p;
        switch (b) {
        case BUF_POS_A: return posA.p; case BUF_POS_B: return posB.p; case BUF_VEL_A: return velA.p; case BUF_VEL_B: return velB.p;
        case BUF_PRES_A: return presA.p; case BUF_PRES_B: return presB.p; case BUF_DENS: return dens.p; case BUF_FORCES: return forces.p;
        case BUF_CELL_START: return cellStart.p; case BUF_CELL_END: return cellEnd.p;
        case BUF_HASH_CUR: return sort.hash(); case BUF_INDEX_CUR: return sort.index();
        default: return nullptr;
        }
    }
    DevBuf errWord; // set by the device-side consistency guard of the scans (GridView::err)
    DevBuf hitBuf, hitCounts; // hit lists shared by the density and force kernels of a step
    HitBuffer hit_buffer() const { return HitBuffer{hitBuf.as<uint32_t>(), hitCounts.as<uint32_t>(), (uint32_t)cap}; }
    // wall-particle deferral (nrs_kernels_tiled.h): this step's wall list, from the near-boundary bit per cell that bt keeps
    WallLists wlist; // its buffers, the scan and the compaction (nrs_wall_list.h)
    WallList wall_view() const { return wlist.view(bt.near_bits(), sort.hash()); }
    int build_wall_list(uint32_t N) { return wlist.build(N, sort, stream, bt.near_bits(), sort.hash()); }
    DevBuf fastQ;             // NRS_FLAG_FAST_ARITH: (p/rho^2, 1/rho) per sorted slot, density kernel -> force kernel
    bool splitClearedCells = false; // this step's split of the coherent re-sort also reset the cell table
    uint64_t nOwned = 0;     // slab decomposition: of the n particles, those this rank owns (the rest are halo copies)
    bool cellsClean = false; // cellStart is all-EMPTY
    bool fusedThisStep = false;
    StageTimer timer; // profiling (nrs_host_profile.h)

    // ---- the state of the particle arrays and of the keys prepared for the next step (nrs_host_state.h) ---------------------------
    // The coupled fields live in `st`: everybody reads them (st.fields()), only its named transitions write them, and array_state()
    // reads the result back as ONE state.  The device pointers they speak about stay here.
    ArrayTracker st;
    ArrayState array_state() const
    {
        return nrs::array_state(st.fields(), ArrayFacts{n, cap, nOwned, exch.on(), exch.host().inplace(), sort.prepared().hash != nullptr,
                                                        sort.prepared().index != nullptr, sort.hash() != nullptr, sort.has_resort()});
    }
    void keys_ready() { sort.keys_written(); st.keys_ready(); } // -> AS_KEYS_READY
    int validate(const char *where) const
    {
        if (array_state() != AS_INVALID) return NRS_OK;
        const ArrayFields &f = st.fields();
        char buf[320];
        snprintf(buf, sizeof(buf), "internal state inconsistent at %s (n %llu cap %llu physN %u owned %llu | hashReady %d rsPending %d countKnown %d "
                 "known %u holes %d inplace %d classified %d slotOrder %d slab %d)", where, (unsigned long long)n, (unsigned long long)cap, f.physN,
                 (unsigned long long)nOwned, f.hashReady, f.rsPending, f.rsCountKnown, f.rsKnownCount, f.holesPending, exch.host().inplace(),
                 f.classifiedValid, f.slotOrderValid, exch.on());
        return fail(NRS_E_STATE, buf);
    }

    bool iisph() const { return cfg.solver == NRS_SOLVER_IISPH; }
    bool sesph() const { return cfg.solver == NRS_SOLVER_SESPH; }
    bool dfsph() const { return cfg.solver == NRS_SOLVER_DFSPH; }
    bool pow2_grid() const { return nrs::pow2_grid(P.gridSize); }

    // ---- which kernels a step launches (nrs_host_plan.h) -----------------------------------------------------------------------
    PlanFacts plan_facts() const
    {
        return PlanFacts{cfg.flags, cfg.solver, KSET == KS_MULLER, std::is_same<R, float>::value, cap, n, geo.q.ok, pow2_grid(), bt.near_bits_valid(), bt.count() != 0,
                         exch.on(), P.numCells};
    }
    Features features() const { return plan_features(plan_facts()); }
    // Chosen at the start of every step (step(), nrs_iisph_predict) and held until its end: a host-driven IISPH step spans three calls.
    // The reference-order repeat of a diverged IISPH step runs by plan_step(stop, true), which solver_step hands over beside it.
    StepPlan plan;
    StepPlan plan_step(int stop, bool ref = false) const { return nrs::plan_step(plan_facts(), stop, ref); }

    // (the members free themselves after this body: the stream has drained by then)
    ~Ctx() override
    {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (ownStream && stream) (void)hipStreamDestroy(stream);
    }

    int alloc_cells()
    {
        const uint64_t C = P.numCells;
        if (C == 0 || C > (1ull << 31)) return fail(NRS_E_INVALID, "numCells out of range");
        NRSCHK(cellStart.alloc(C * 4));
        NRSCHK(cellEnd.alloc(C * 4));
        NRSCHK(bt.alloc_cells(C));
        if (cellsAllocated != C) {
            cellsClean = false;
            HIPCHK(hipMemsetAsync(cellEnd.p, 0, C * 4, stream));
            NRSCHK(bt.zero_cell_ends(C, stream));
            cellsAllocated = (uint32_t)C;
        }
        return NRS_OK;
    }

    int init(const nrs_config &c, const void *params) override
    {
        cfg = c;
        cap = c.capacity;
        if (cap == 0 || cap > (uint64_t)HIT_INDEX) return fail(NRS_E_INVALID, "capacity must be in 1..2^27-1");
        std::memcpy(&PU, params, sizeof(PU));
        derive_kernel_params();
        const size_t v = sizeof(T4) * cap, s = sizeof(R) * cap;
        NRSCHK(posA.alloc(v)); NRSCHK(posB.alloc(v)); NRSCHK(velA.alloc(v)); NRSCHK(velB.alloc(v));
        NRSCHK(presA.alloc(s)); NRSCHK(presB.alloc(s)); NRSCHK(dens.alloc(s)); NRSCHK(forces.alloc(v));
        HIPCHK(hipMemsetAsync(presA.p, 0, s, stream));
        HIPCHK(hipMemsetAsync(presB.p, 0, s, stream));
        HIPCHK(hipMemsetAsync(dens.p, 0, s, stream));
        HIPCHK(hipMemsetAsync(forces.p, 0, v, stream));
        NRSCHK(ps.init(cfg.solver, cap, stream));
        const Features ft = features();
        if (ft.lists) {
            NRSCHK(hitBuf.alloc((size_t)HIT_CAP * cap * 4));
            NRSCHK(hitCounts.alloc((size_t)cap * 4));
            NRSCHK(qpos.alloc(((size_t)cap + 4) * sizeof(qword_t)));
            if (sesph()) NRSCHK(gatherPos.alloc((size_t)cap * 2 * sizeof(T4)));
        }
        if (ft.fast) NRSCHK(fastQ.alloc((size_t)cap * sizeof(FastPair)));
        NRSCHK(errWord.alloc(8)); // [0] run guard of the scans, [1] IISPH: a gathered value went non-finite (IisphArrays::nonFinite)
        HIPCHK(hipMemsetAsync(errWord.p, 0, 8, stream));
        NRSCHK(red.init(stream));
        NRSCHK(sort.init(cap, ft.resort, stream));
        exch.init(cap, stream);
        NRSCHK(alloc_cells());
        return NRS_OK;
    }

    // a host-driven IISPH step (nrs_iisph_predict .. nrs_iisph_finish) holds hit lists, factors and a halo budget that belong to the
    // arrays, grid and cuts it was predicted on: everything that would change those is refused until it is finished (or abandoned
    // by uploading particles)
    int refuse_mid_iisph(const char *what) const
    {
        if (!ps.host_step()) return NRS_OK;
        char buf[200];
        snprintf(buf, sizeof(buf), "%s while a host-driven IISPH step is in progress (nrs_iisph_finish first, or upload particles to abandon it)", what);
        return fail(NRS_E_STATE, buf);
    }
    int set_params(const void *params) override
    {
        NRSCHK(refuse_mid_iisph("nrs_set_params"));
        Params<R> q;
        std::memcpy(&q, params, sizeof(q));
        // the keys the fused force kernel left for the next step depend on the grid only (a new time step or viscosity
        // does not invalidate them: the reference calls setParameters every update(), the CFL variant with a new dt)
        const bool sameGrid = std::memcmp(PU.gridSize, q.gridSize, sizeof(PU.gridSize)) == 0 && q.numCells == PU.numCells &&
                              std::memcmp(PU.worldOrigin, q.worldOrigin, sizeof(PU.worldOrigin)) == 0 &&
                              std::memcmp(PU.cellSize, q.cellSize, sizeof(PU.cellSize)) == 0;
        if (!sameGrid) NRSCHK(invalidate_grid_state());
        const uint32_t cellsBefore = P.numCells;
        const StaleConstants stale = stale_after_params(params_key(PU), params_key(q)); // (the host classes set the parameters every step)
        ps.params_changed(stale);
        PU = q;
        if (!sameGrid && exch.on()) exch.choose_window(PU.gridSize, true);
        derive_kernel_params();
        const bool regrid = P.numCells != cellsBefore;
        if (regrid) NRSCHK(alloc_cells());
        if (!sameGrid) NRSCHK(rebuild_boundary_tables()); // the boundary hashes / cell table depend on origin, cell size and extents
        return NRS_OK;
    }
    // The grid (origin, cell size or extents) is about to change: every key computed for the old grid is void — the
    // keys the fused kernel prepared for the next step, the split of the coherent re-sort, the slot order, a slab
    // classification — and the cell table has to be reset in full (k_clear_cells undoes only cells of the OLD keys).
    int invalidate_grid_state()
    {
        NRSCHK(compact_holes());
        st.grid_changed();
        cellsClean = false;
        ++gridGen;
        return NRS_OK;
    }
    static ParamsKey params_key(const Params<R> &p)
    {
        return ParamsKey{(double)p.timestep, (double)p.particleMass, (double)p.restDensity, (double)p.interactionRadius, (double)p.kpoly,
                         (double)p.kpoly_grad, (double)p.kpress_grad};
    }
    int get_params(void *params) override
    {
        std::memcpy(params, &PU, sizeof(PU));
        return NRS_OK;
    }

    int upload(const void *pos4, const void *vel4, const void *pres, uint64_t first, uint64_t count) override
    {
        NRSCHK(validate("nrs_upload_particles"));
        if (first + count > cap) return fail(NRS_E_CAPACITY, "upload exceeds capacity");
        if (track.on && count && !pos4) return fail(NRS_E_INVALID, "pos4 is NULL"); // (tracking: refused before the ids are handed out)
        if (track.on) NRSCHK(track_new_slots(track_fresh_after_upload(n, first, count))); // slots at or above the old n are new particles
        NRSCHK(compact_holes());
        if (count) {
            if (!pos4) return fail(NRS_E_INVALID, "pos4 is NULL");
            HIPCHK(hipMemcpyAsync(posA.as<T4>() + first, pos4, sizeof(T4) * count, hipMemcpyHostToDevice, stream));
            if (vel4) HIPCHK(hipMemcpyAsync(velA.as<T4>() + first, vel4, sizeof(T4) * count, hipMemcpyHostToDevice, stream));
            else HIPCHK(hipMemsetAsync(velA.as<T4>() + first, 0, sizeof(T4) * count, stream));
            if (pres) HIPCHK(hipMemcpyAsync(presA.as<R>() + first, pres, sizeof(R) * count, hipMemcpyHostToDevice, stream));
            else HIPCHK(hipMemsetAsync(presA.as<R>() + first, 0, sizeof(R) * count, stream));
            NRSCHK(ps.kv_zero(first, count, stream));
            HIPCHK(hipStreamSynchronize(stream)); // the caller may reuse its host buffers on return
        }
        if (first + count > n) n = first + count;
        ++particleGen;
        if (exch.on()) nOwned = n; // (until the next partition says otherwise)
        midStep = false;
        ps.abandon_host_step(); // new particles abandon a host-driven IISPH step that was in progress
        st.to_fresh();
        return NRS_OK;
    }
    int set_n(uint64_t nn) override
    {
        NRSCHK(validate("nrs_set_num_particles"));
        if (nn > cap) return fail(NRS_E_CAPACITY, "n exceeds capacity");
        if (track.on) NRSCHK(track_new_slots(track_fresh_after_set_n(n, nn))); // growing: fresh ids; shrinking drops the tail
        NRSCHK(compact_holes());
        if (nn != n) st.to_fresh();
        if (nn != n) ++particleGen;
        if (nn != n) ps.abandon_host_step(); // (the hit lists of a predicted step belong to the old particle set)
        n = nn;
        if (exch.on()) nOwned = n;
        return NRS_OK;
    }
    uint64_t get_n() override { return n; }

    // ---- boundaries: the state and the builds live in bt (nrs_boundary_tables.h); here: what the context tells it, and the grid rule ---
    uint32_t sort_end_bit() const { return sort_key_bits(P.numCells); }
    BoundaryGrid<R> boundary_grid()
    {
        return BoundaryGrid<R>{P, sort_end_bit(), features().listKernels && pow2_grid(), stream, [this] { return wlist.ensure(cap, stream); }};
    }
    // the tables at the uploaded positions, on the current grid (the boundary hashes / cell table depend on origin, cell size and extents)
    int rebuild_boundary_tables()
    {
        if (!bt.count()) return NRS_OK;
        NRSCHK(alloc_cells());
        return bt.build_at_rest(boundary_grid());
    }
    int set_boundary_bodies(const uint32_t *bodyOf, uint64_t nbGiven, uint32_t nbodies) override
    {
        NRSCHK(refuse_mid_iisph("nrs_set_boundary_bodies"));
        if (nbodies && visc.wall_friction())
            return fail(NRS_E_STATE, "nrs_set_boundary_bodies on a context with implicit wall friction (nrs_dfsph_set_viscosity, nu_boundary > 0)");
        ++boundaryGen;
        return bt.set_bodies(bodyOf, nbGiven, nbodies, exch.on(), boundary_grid());
    }
    int set_body_velocity(uint32_t body, const double *v, const double *omega) override { return bt.set_body_velocity(body, v, omega); }
    int set_body_pose(uint32_t body, const double *x, const double *q) override { return bt.set_body_pose(body, x, q); }
    int get_body_pose(uint32_t body, double *x, double *q) override { return bt.get_body_pose(body, x, q); }
    int advance_bodies_and_rebuild() { return bt.advance_and_rebuild(P, (double)PU.timestep, sort_end_bit(), timer, profMask, stream); }

    // Everything that can be refused is decided from the incoming arrays before anything is stored: a refused call changes nothing.
    int set_boundaries(const void *bi4, const void *vbi, uint64_t nbNew, int update_grid) override
    {
        NRSCHK(refuse_mid_iisph("nrs_set_boundaries"));
        if (nbNew > (uint64_t)HIT_INDEX) return fail(NRS_E_INVALID, "too many boundary particles (max 2^27-1)");
        if (nbNew && (!bi4 || !vbi)) return fail(NRS_E_INVALID, "bi4/vbi is NULL");
        const bool regrid = nbNew && update_grid;
        AabbGrid<R> g;
        if (regrid) { // BBMin/BBMax (sph_cuda.cu:461-505) + SPH::updateGrid (sph.cpp:313-337): nrs_host_grid.h
            R mn[3], mx[3];
            aabb_of_points((const R *)bi4, nbNew, mn, mx);
            NRSCHK(grid_from_aabb(mn, mx, PU.interactionRadius, g));
        }
        bt.set_particles(bi4, vbi, nbNew); // (a new set of boundary particles has no body assignment)
        ++boundaryGen;
        if (!nbNew) return NRS_OK;
        if (regrid) {
            NRSCHK(invalidate_grid_state());
            for (int a = 0; a < 3; ++a) { PU.worldOrigin[a] = g.origin[a]; PU.gridSize[a] = g.size[a]; }
            PU.numCells = g.numCells;
            if (exch.on()) exch.choose_window(PU.gridSize, true);
            derive_kernel_params();
        }
        return rebuild_boundary_tables();
    }

    // ---- profiling helpers ------------------------------------------------------------------------
    int ev_begin(int stage, bool cont = false) { return timer.begin(stage, cont, profMask, stream); }
    int ev_end() { return timer.end(stream); }
    int set_profiling(uint32_t mask) override
    {
        NRSCHK(timer.reset(stream));
        profMask = mask;
        return NRS_OK;
    }
    int stage_ms(int stage, float *ms, uint32_t *launches) override { return timer.read(stage, ms, launches, stream); }

    GridView<R> grid_view() const
    {
        GridView<R> G;
        G.cellStart = cellStart.as<uint32_t>(); G.cellEnd = cellEnd.as<uint32_t>();
        G.bCellStart = bt.cell_start(); G.bCellEnd = bt.cell_end();
        G.sB = bt.sorted();
        G.actLo = INT_MIN;
        G.actHi = INT_MAX;
        G.nSorted = (uint32_t)n;
        G.err = errWord.as<uint32_t>();
        G.qpos = plan.quant ? qpos.as<qword_t>() : (const qword_t *)nullptr;
        G.qT = geo.q.qT;
        G.qc = geo.q.qc;
        return G;
    }
    // what the step is now, for a chain of ps (nrs_solvers.h): built once per chain, from the plan of the step in progress
    SolverStep<R> solver_step(int stop)
    {
        const uint32_t N = (uint32_t)n;
        return SolverStep<R>{P, plan, plan_step(stop, true), grid_view(), geo.thr, hit_buffer(), wall_view(),
                             SortedArrays<R>{posB.as<T4>(), velB.as<T4>(), dens.as<R>(), presB.as<R>(), N}, presA.as<R>(), sort.index(),
                             errWord.as<uint32_t>() + 1 /* (second word of the error buffer) */, exch.on(), exch.max_iters(), bt.moving_step(),
                             bt.wall_velocities(), maxIters, &lastIters, &timer, profMask, stream};
    }

    // hash → sort → cell ranges + reorder: common prefix of both solvers
    int stage_prefix(int stop)
    {
        const uint32_t N = (uint32_t)n;
        const dim3 g(nblocks(N)), b(BLOCK);
        // which of merge, full sort or compact-first this step takes (nrs_host_state.h); the launches below read the choice
        const SortPrefix c = sort.choose_prefix(st.fields(), stop, n);
        if (c.compactFirst) NRSCHK(compact_holes()); // also drops the prepared keys: hash and sort from scratch below
        if (c.useKeys) { // keys/values of this step were produced by the previous step's fused force kernel
            sort.take_prepared();
        } else {
            sort.take_fresh();
            NRSCHK(ev_begin(NRS_STAGE_HASH));
            hipLaunchKernelGGL((k_hash<R>), g, b, 0, stream, P, posA.as<T4>(), sort.hash(), sort.index(), N);
            NRSCHK(ev_end());
        }
        st.drop_prepared_keys(); // (consumed by this step)
        if (stop == NRS_STAGE_HASH) return NRS_OK;

        const uint64_t *merged = nullptr; // the u64 pairs of the coherent re-sort, or null after the full sort
        NRSCHK(ev_begin(NRS_STAGE_SORT, c.resort));
        NRSCHK(sort.sort_keys(c, N, sort_end_bit(), &merged));
        NRSCHK(ev_end());
        if (stop == NRS_STAGE_SORT) return NRS_OK;

        NRSCHK(ev_begin(NRS_STAGE_REORDER));
        if (!cellsClean) HIPCHK(hipMemsetAsync(cellStart.p, 0xff, (size_t)P.numCells * 4, stream));
        cellsClean = false;
        st.holes_consumed(); // the gather below reads only live slots
        const uint32_t *nearB = plan.wallTiles ? bt.near_bits() : (const uint32_t *)nullptr;
        qword_t *qp = plan.quant ? qpos.as<qword_t>() : (qword_t *)nullptr;
        if (merged)
            hipLaunchKernelGGL((k_reorder_merged<R>), g, b, 0, stream, merged, sort.hash(), sort.index(), posA.as<T4>(), velA.as<T4>(),
                               iisph() ? presA.as<R>() : (const R *)nullptr, posB.as<T4>(), velB.as<T4>(), presB.as<R>(),
                               cellStart.as<uint32_t>(), cellEnd.as<uint32_t>(), iisph() ? ps.inverse_slots() : (uint32_t *)nullptr, N,
                               nearB, wlist.tile_counts(), wlist.slot_masks(), geo.q.qc, qp);
        else
            hipLaunchKernelGGL((k_reorder<R>), g, b, 0, stream, sort.hash(), sort.index(), posA.as<T4>(), velA.as<T4>(),
                               iisph() ? presA.as<R>() : (const R *)nullptr, posB.as<T4>(), velB.as<T4>(), presB.as<R>(),
                               cellStart.as<uint32_t>(), cellEnd.as<uint32_t>(), iisph() ? ps.inverse_slots() : (uint32_t *)nullptr, N,
                               nearB, wlist.tile_counts(), wlist.slot_masks(), geo.q.qc, qp);
        if (iisph() && (cfg.flags & NRS_FLAG_IISPH_SELF_BY_SLOT)) // Q5 off: the pressure kernels skip j == own slot
            hipLaunchKernelGGL(k_identity, g, b, 0, stream, ps.inverse_slots(), N);
        if (dfsph()) { // the warm-start inputs of the step, K_prev and Kv_prev, into sorted order
            hipLaunchKernelGGL((k_gather_scalar<R>), g, b, 0, stream, presA.as<R>(), sort.index(), presB.as<R>(), N);
            ps.kv_gather(sort.index(), N, stream);
        }
        NRSCHK(ev_end());
        if (track.on) { // id, birth and the record into sorted order: one launch, an entry of its own in the reorder stage's count
            NRSCHK(ev_begin(NRS_STAGE_REORDER));
            track.template gather<R>(sort.index(), N, stream);
            NRSCHK(ev_end());
        }
        return NRS_OK;
    }

    // Somebody wants to look at (or re-partition) the particle arrays while they still have the holes of an in-place slab
    // partition: compact them now (stable) and forget the prepared re-sort; the next step hashes and sorts from scratch.
    int compact_holes()
    {
        if (!st.fields().holesPending) return NRS_OK;
        const uint32_t NP = st.fields().physN, nTiles = nblocks(NP);
        st.holes_compacted();
        if (!NP) return NRS_OK;
        NRSCHK(sort.scan_holes(NP));
        hipLaunchKernelGGL((k_holes_compact<R>), dim3(nTiles), dim3(BLOCK), 0, stream, sort.prepared().hash, sort.offsets_dead(), posA.as<T4>(), velA.as<T4>(),
                           posB.as<T4>(), velB.as<T4>(), NP);
        HIPCHK(hipGetLastError());
        std::swap(posA.p, posB.p);
        std::swap(velA.p, velB.p);
        return NRS_OK;
    }

    // first half of the next step's sort, queued right behind the kernel that produced the prepared keys and counted
    // the movers per tile: scan of the tile counts (total to the host) + stable split into movers / stayers
    int queue_resort_split(uint32_t N)
    {
        NRSCHK(ev_begin(NRS_STAGE_SORT));
        NRSCHK(sort.scan_movers(nblocks(N), false));
        const bool clear = sparse_cell_table(P.numCells, n); // the step's cell-table reset rides along (see step())
        NRSCHK(sort.split(SplitFrom::SORTED, N, clear ? cellStart.as<uint32_t>() : (uint32_t *)nullptr));
        splitClearedCells = clear;
        st.split_queued();
        NRSCHK(ev_end());
        return NRS_OK;
    }

    template <bool HAS_B> int sesph_tail(int stop)
    {
        const uint32_t N = (uint32_t)n;
        const dim3 g(nblocks(N)), b(BLOCK);
        GridView<R> G = grid_view();
        if (exch.on()) { G.actLo = exch.cuts().lo - 1; G.actHi = exch.cuts().hi + 1; } // density is also needed one cell beyond the cuts
        // the density kernel's hit lists are handed to the force kernel when both run in this call
        HitBuffer hb = hit_buffer();
        hb.gpos = gatherPos.p; hb.gvel = gatherPos.as<T4>() + 1; hb.svel = velB.p; // (the two records of a slot side by side: GATHER_STRIDE)
        if (plan.fast && !plan.staged) hb.fast = fastQ.as<FastPair>(); // (the staged kernel writes fastQ through its own argument)
        const HitBuffer *share = plan.lists ? &hb : nullptr;
        const WallList wv = wall_view();
        const WallList *walls = plan.walls ? &wv : nullptr;
        if (plan.walls) { // (timed with the reorder stage, whose tile counts it finishes: the density stage is its one launch)
            NRSCHK(ev_begin(NRS_STAGE_REORDER, true));
            NRSCHK(build_wall_list(N));
            NRSCHK(ev_end());
        }
        NRSCHK(ev_begin(NRS_STAGE_DENSITY));
        if (plan.ref) {
            hipLaunchKernelGGL((k_density_ref<R, KSET, HAS_B>), g, b, 0, stream, P, G, posB.as<T4>(), dens.as<R>(), presB.as<R>(), N);
        } else if (plan.staged) {
            if constexpr (std::is_same<R, float>::value)
                launch_density_staged<KSET, HAS_B>(stream, P, G, geo.thr, share, plan.fast, posB.as<T4>(), dens.as<R>(), presB.as<R>(),
                                                   plan.fast ? fastQ.as<FastPair>() : (FastPair *)nullptr, N);
        } else {
            launch_density_tiled<R, KSET, HAS_B>(stream, P, G, geo.thr, share, posB.as<T4>(), dens.as<R>(), presB.as<R>(), N, walls);
        }
        if (exch.on()) { G.actLo = exch.cuts().lo; G.actHi = exch.cuts().hi; }
        NRSCHK(ev_end());
        if (stop == NRS_STAGE_DENSITY) return NRS_OK;
        // A full step on the production kernels fuses forces + integrate + next-step hash into one launch that
        // writes the new state straight into the A ("current") arrays, which reorder has finished reading.
        NRSCHK(ev_begin(NRS_STAGE_FORCES));
        FusedOut<R> fo{};
        if (plan.keys) {
            fo.newPos = posA.as<T4>(); fo.newVel = velA.as<T4>();
            fo.hash = sort.next_keys().hash; fo.index = sort.next_keys().index;
            fo.slab = exch.cuts();
            if (plan.resort || plan.classify) {
                NRSCHK(sort.clean_tile_counts());
                fo.prevHash = sort.hash();
                fo.tileMovers = sort.tile_movers();
            }
            st.classification_dropped();
            if (plan.classify) {
                SlabClassify sc;
                NRSCHK(exch.classify_targets(N, sc));
                fo.slabFlags = sc.flags;
                fo.slabBlockCounts = sc.blockCounts;
                fo.slabBlocks = sc.blocks;
                fo.tileDead = sort.tile_dead();
                st.classified(N);
                sort.tile_counts_written(); // until a pack's scan consumes the tile counts
            }
        }
        const FusedOut<R> *fused = plan.keys ? &fo : nullptr;
        T4 *out = plan.keys ? (T4 *)nullptr : forces.as<T4>();
        if (plan.ref) {
            hipLaunchKernelGGL((k_forces_ref<R, KSET, SURF, HAS_B>), g, b, 0, stream, P, G, posB.as<T4>(), velB.as<T4>(),
                               dens.as<R>(), presB.as<R>(), out, N);
        } else if (plan.fast) {
            if constexpr (std::is_same<R, float>::value && KSET == KS_MULLER)
                launch_forces_fast<SURF, HAS_B>(stream, P, G, hb, posB.as<T4>(), velB.as<T4>(), dens.as<R>(), presB.as<R>(),
                                                fastQ.as<FastPair>(), out, fused, N);
        } else {
            launch_forces_tiled<R, KSET, SURF, HAS_B>(stream, P, G, geo.thr, share, posB.as<T4>(), velB.as<T4>(), dens.as<R>(), presB.as<R>(), out,
                                                      fused, N, walls);
        }
        if (plan.keys) {
            if (!exch.on()) keys_ready();
            else sort.keys_written(); // a slab run re-partitions the arrays before the next step (AS_SLOT_ORDER)
            fusedThisStep = true;
        }
        NRSCHK(ev_end());
        if (plan.resort) NRSCHK(queue_resort_split(N));
        if (stop == NRS_STAGE_FORCES || plan.keys) return NRS_OK;
        NRSCHK(ev_begin(NRS_STAGE_INTEGRATE));
        hipLaunchKernelGGL((k_integrate<R>), g, b, 0, stream, P, posB.as<T4>(), velB.as<T4>(), forces.as<T4>(), N);
        NRSCHK(ev_end());
        return NRS_OK;
    }

    int reduce_max(int which, double *out) override
    {
        if (!n) { *out = 0; return NRS_OK; }
        NRSCHK(compact_holes());
        if (which == 0) return red.template max_of<false>(dens.p, (uint32_t)n, out);
        return red.template max_of<true>(velA.p, (uint32_t)n, out);
    }

    // ---- the pressure solvers: ps (nrs_solvers.h) has the settings and the chains; here: the forwards, and what frames a chain --------
    int pcisph_configure(double eta, uint32_t minIters, double spacing, double delta) override { return ps.pcisph_configure(eta, minIters, spacing, delta); }
    int pbf_configure(double eta, uint32_t minIters, double relaxation, double xsph) override { return ps.pbf_configure(eta, minIters, relaxation, xsph); }
    int pbf_set_tensile(double k, double dq) override { return ps.pbf_set_tensile(P, k, dq, stream); }
    int pbf_set_vorticity(double epsV) override { return ps.pbf_set_vorticity(epsV); }
    int dfsph_configure(double eta, uint32_t minIters, double etaV, uint32_t minItersV, int warm) override { return ps.dfsph_configure(eta, minIters, etaV, minItersV, warm); }
    int set_surface_akinci(double gamma, double beta) override { return ps.set_surface_akinci(gamma, beta); }
    int dfsph_set_viscosity(double nu, double nuB, double tol, uint32_t minIters, uint32_t maxIters) override
    {
        return ps.dfsph_set_viscosity(nu, nuB, tol, minIters, maxIters, bt.has_bodies());
    }
    int dfsph_viscosity_info(int *on, uint32_t *iterations, double *residual, double *rhsNorm) override
    {
        if (!dfsph()) return fail(NRS_E_STATE, "nrs_dfsph_viscosity_info on a context that is not DFSPH");
        return visc.info(stream, on, iterations, residual, rhsNorm);
    }

    // f(std::true_type) with boundary particles, f(std::false_type) without: the one place a launch chain learns HAS_B
    template <typename F> int with_walls(F &&f) { return bt.count() ? f(std::true_type{}) : f(std::false_type{}); }
    // The last launch of an IISPH, PCISPH, PBF or DFSPH step, inside the stage the caller opened: like the fused SESPH force kernel it
    // also writes the next step's sort keys (pl.keys) and counts the movers per tile (pl.resort).  launch(hash, index, prevHash,
    // tileMovers) gets where those go, or nulls; the stage ends behind it, the keys are ready and the split is queued.  pl: the plan
    // the chain runs by — the step's, or the one of IISPH's repeat in reference order, which leaves no keys.
    template <typename Launch> int launch_last(const StepPlan &pl, Launch &&launch)
    {
        const KeyPair next = pl.keys ? sort.next_keys() : KeyPair{nullptr, nullptr};
        if (pl.resort) NRSCHK(sort.clean_tile_counts());
        launch(next.hash, next.index, pl.resort ? (const uint32_t *)sort.hash() : (const uint32_t *)nullptr, pl.resort ? sort.tile_movers() : (uint32_t *)nullptr);
        NRSCHK(ev_end());
        if (pl.keys) keys_ready();
        if (pl.resort) NRSCHK(queue_resort_split((uint32_t)n));
        return NRS_OK;
    }
    auto last_launch()
    {
        return [this](const StepPlan &pl, auto &&launch) { return this->launch_last(pl, launch); };
    }
    // The head of an IISPH, PCISPH, PBF or DFSPH chain: this step's wall list, timed with the reorder stage, whose tile counts it
    // finishes.  The one neighbourhood scan of the step follows it (ps).
    int wall_list_of_step()
    {
        if (!plan.walls) return NRS_OK;
        NRSCHK(ev_begin(NRS_STAGE_REORDER, true));
        NRSCHK(build_wall_list((uint32_t)n));
        return ev_end();
    }
    // everything behind the reorder of a step
    template <bool HAS_B> int tail(int stop)
    {
        if (sesph()) return sesph_tail<HAS_B>(stop);
        if (plan.watch) HIPCHK(hipMemsetAsync(errWord.as<uint32_t>() + 1, 0, 4, stream)); // (IISPH: SolverStep::nonFinite)
        NRSCHK(wall_list_of_step());
        return ps.template tail<HAS_B>(solver_step(stop), stop, last_launch());
    }

    // ---- host-driven IISPH step (multi-GPU: the loop exit needs the average over ALL ranks) ---------------------------------
    int iisph_phase(int phase, double *sum, uint64_t *count) override
    {
        if (!iisph()) return fail(NRS_E_STATE, "not an IISPH context");
        NRSCHK(validate("nrs_iisph_*"));
        if (phase == 0) { // predict
            if (midStep || ps.host_step()) return fail(NRS_E_STATE, "a step is already in progress");
            if (inflow.active()) NRSCHK(apply_inflow());
            if (n == 0) return NRS_OK;
            fusedThisStep = false; splitClearedCells = false;
            plan = plan_step(0);
            NRSCHK(advance_bodies_and_rebuild());
            NRSCHK(stage_prefix(0));
            NRSCHK(wall_list_of_step());
            return with_walls([&](auto hasB) { return ps.template host_predict<hasB>(solver_step(0)); });
        }
        if (!ps.host_step()) return fail(NRS_E_STATE, "nrs_iisph_predict first");
        if (phase == 1) return with_walls([&](auto hasB) { return ps.template host_iterate<hasB>(solver_step(0), sum, count); });
        // finish
        NRSCHK(with_walls([&](auto hasB) { return ps.template host_finish<hasB>(solver_step(0), last_launch()); }));
        HIPCHK(hipGetLastError());
        NRSCHK(end_of_step());
        ps.host_step_ended();
        return NRS_OK;
    }
    // ---- slab decomposition: the exchange itself lives in exch (nrs_slab_exchange.h; its kernels: nrs_kernels_slab.h; the host
    // decisions: nrs_host_slab.h); here: the refusals, and what a call does to n, nOwned and the state of the particle arrays ----------
    int slab_configure(int lo, int hi, int halo) override
    {
        NRSCHK(refuse_mid_iisph("nrs_slab_configure"));
        NRSCHK(slab_refuse_configure(cfg.solver, bt.has_bodies(), lo, hi, halo));
        if (inflow.configured()) return inflow_refuse_slab();
        if (track.on) return track_refuse_slab_configure();
        bool cutsChanged = false;
        exch.configure(lo, hi, halo, &cutsChanged);
        // the last force kernel classified (and marked dead keys) for the old cuts: partition the slow way once
        if (st.fields().classifiedValid && cutsChanged) st.cuts_changed();
        nOwned = n;
        // cell-table window of this rank (see PU / P): re-chosen only when the slab no longer fits the current one
        const uint32_t cellsBefore = P.numCells, baseBefore = P.numBodies;
        if (exch.choose_window(PU.gridSize, false)) {
            NRSCHK(invalidate_grid_state());
            derive_kernel_params();
            if (P.numCells != cellsBefore || P.numBodies != baseBefore) {
                cellsAllocated = 0; // (same size, other columns: the tables still have to be reset)
                NRSCHK(alloc_cells());
                NRSCHK(rebuild_boundary_tables());
            }
        }
        return NRS_OK;
    }
    uint64_t num_owned() override { return exch.on() ? nOwned : n; }
    int slab_histogram(int lo0, uint32_t nbins, uint32_t *out) override
    {
        if (!nbins || !out) return fail(NRS_E_INVALID, "bad histogram request");
        NRSCHK(compact_holes());
        return exch.histogram(P, posA.as<T4>(), n, lo0, nbins, out);
    }

    int slab_pack(void *sendL, void *sendR, uint64_t mcap, uint32_t *counts) override
    {
        NRSCHK(validate("nrs_slab_pack"));
        if (!exch.on()) return fail(NRS_E_STATE, "nrs_slab_configure first");
        if (midStep) return fail(NRS_E_STATE, "state is mid-update");
        if (mcap == 0 || mcap > (uint64_t)HIT_INDEX) return fail(NRS_E_INVALID, "bad message capacity");
        NRSCHK(finish_pack());   // (a pack right behind a pack whose totals nobody has looked at yet)
        NRSCHK(compact_holes()); // (a pack right after a pack/unpack without a step in between)
        if (ps.host_step()) return fail(NRS_E_STATE, "a host-driven IISPH step is in progress");
        if (iisph() && n) // the warm-start pressure travels in vel.w (k_pressure_to_velw)
            hipLaunchKernelGGL((k_pressure_to_velw<R>), dim3(nblocks(n)), dim3(BLOCK), 0, stream, velA.as<T4>(), presA.as<R>(), (uint32_t)n);
        const uint32_t N = (uint32_t)n;
        const SlabChoice ch = choose_form(SlabFacts{st.fields().classifiedValid, st.fields().slotOrderValid, sort.has_resort(), sort.hash() != nullptr,
                                                    sort.prepared().hash != nullptr, sort.prepared().hash != sort.hash(), st.fields().classifiedN, N, RESORT_MIN_PARTICLES});
        // count -> scan -> scatter, the headers, the totals on their way to the host, in place the split; nothing waits: the totals
        // are read back by finish_pack()
        NRSCHK(exch.pack(P, posA.as<T4>(), velA.as<T4>(), posB.as<T4>(), velB.as<T4>(), N, sendL, sendR, mcap, ch, sort));
        if (counts) { // the caller wants the counts now: that is the synchronisation it asked for
            NRSCHK(finish_pack());
            std::memcpy(counts, exch.host().totals, ST_COUNT * sizeof(uint32_t));
        }
        return NRS_OK;
    }
    // ---- the host half of nrs_slab_pack, run when the stream totals are needed: what they mean for the arrays -----------------------
    int finish_pack()
    {
        SlabFinish f;
        const int rc = exch.finish(f); // (nothing pending, or the wait failed: nothing stored)
        if (!f.stored) return rc;
        const uint32_t packedN = exch.host().N;
        st.to_fresh();
        if (f.form != SlabForm::COMPACT) {
            // the prepared keys / values hold key and slot of every live slot, 0xffffffff marks the dead ones; arrivals are added to the mover
            // count by nrs_slab_unpack
            st.to_holes(packedN, f.movers);
        } else {
            if (packedN) { std::swap(posA.p, posB.p); std::swap(velA.p, velB.p); }
            else sort.pack_targets_empty();
            st.pack_hashed(packedN != 0); // k_slab_scatter hashed the particles that stay (with the current parameters)
        }
        n = f.n;
        nOwned = n;
        return rc; // (NRS_E_CAPACITY: reported with the counts stored)
    }
    int settle() override { return finish_pack(); }
    int slab_last_counts(uint32_t *counts) override
    {
        NRSCHK(finish_pack());
        std::memcpy(counts, exch.host().totals, ST_COUNT * sizeof(uint32_t));
        return NRS_OK;
    }

    int slab_unpack(const void *recvL, const void *recvR, uint64_t mcap) override
    {
        NRSCHK(validate("nrs_slab_unpack"));
        NRSCHK(refuse_mid_iisph("nrs_slab_unpack"));
        if (!exch.on()) return fail(NRS_E_STATE, "nrs_slab_configure first");
        // ONE host synchronisation for the exchange: the wait for the headers of the received messages also covers the stream totals
        // of the pack (finish_pack)
        const uint32_t *hL = nullptr, *hR = nullptr;
        NRSCHK(exch.read_headers(recvL, recvR, &hL, &hR));
        NRSCHK(finish_pack());
        SlabArrivals ar;
        NRSCHK(exch.arrivals(hL, hR, n, st.fields().physN, st.fields().holesPending, mcap, ar));
        // compacting form with a re-sort: the append extends the compacted old keys and the tile counts of the scatter
        const bool compactResort = exch.host().form == SlabForm::COMPACT && exch.host().resort;
        NRSCHK(exch.append(P, ar, recvL, recvR, mcap, posA.as<T4>(), velA.as<T4>(), sort, compactResort, ar.inplace ? st.fields().rsKnownCount : 0u));
        nOwned = ar.nOwned;
        n = ar.n;
        if (iisph() && n)
            hipLaunchKernelGGL((k_velw_to_pressure<R>), dim3(nblocks(n)), dim3(BLOCK), 0, stream, velA.as<T4>(), presA.as<R>(), (uint32_t)n);
        // pack + unpack have written the radix keys/values of every local particle
        sort.pack_wrote_every_key();
        st.arrivals_appended(ar.inplace, (uint32_t)ar.arrivals);
        if (!ar.inplace && st.fields().hashReady && compactResort && n >= RESORT_MIN_PARTICLES) {
            // coherent re-sort: the owned particles that stayed in their cell are still in sorted order
            // (the partition and the append have counted the movers of every tile of the new arrays)
            const uint32_t N = (uint32_t)n;
            NRSCHK(sort.scan_movers(nblocks(N), false));
            NRSCHK(sort.split(SplitFrom::PACKED, N, nullptr));
            st.split_queued_known(exch.host().totals[ST_CHANGED] + ar.start[5]); // everything appended is a mover, and the partition counted the cell changers
        }
        exch.unpack_done();
        return NRS_OK;
    }

    void resort_stats(uint64_t *steps, uint64_t *fallbacks) override
    {
        if (steps) *steps = sort.stats().steps;
        if (fallbacks) *fallbacks = sort.stats().fallbacks;
    }
    // which statistic an id means on this context, or its refusal: route_stat (nrs_host_solver.h); the device work on a solver's buffer
    // is ps's, on the hit lists red's
    StatFacts stat_facts() const
    {
        return StatFacts{cfg.solver, exch.host().packed, ps.pbfSt.errPending != 0, !(ps.pciSt.lastErr < 0.0), ps.dfSt.denN, ps.dfSt.divN, hitCounts.p != nullptr, n != 0, midStep};
    }
    int get_stat(int which, double *out) override
    {
        StatRoute r;
        NRSCHK(route_stat(which, stat_facts(), r));
        if (r.formMaxFirst) {
            NRSCHK(ps.form_pending_max());
            NRSCHK(route_stat(which, stat_facts(), r)); // again, on the maximum just formed: "no PBF solve yet" is tested on that value
        }
        switch (r.kind) {
        case STAT_MOVER_COUNT: *out = sort.stats().lastMovers; return NRS_OK;
        case STAT_SLAB_FORM: *out = (int)exch.host().form; return NRS_OK;
        case STAT_PBF_ERROR:
        case STAT_PCI_ERROR: *out = ps.pciSt.lastErr; return NRS_OK;
        case STAT_PBF_EPS: *out = (double)ps.pbfSt.eps(); return NRS_OK;
        case STAT_PCI_DELTA: *out = (double)ps.pciSt.delta(); return NRS_OK;
        case STAT_DFSPH_DIV_ITERS: *out = (double)ps.dfSt.divIters; return NRS_OK;
        case STAT_DFSPH_MAX: return ps.dfsph_error(r.divergence, false, r.count, out);
        case STAT_DFSPH_AVG: return ps.dfsph_error(r.divergence, true, r.count, out);
        case STAT_HIT_OVERFLOW:
        case STAT_HIT_MEAN:
        case STAT_HIT_MAX:
        case STAT_HIT_UNSTAGED: break;
        }
        const uint32_t N = (uint32_t)n;
        unsigned long long h[4] = {0, 0, 0, 0};
        NRSCHK(red.hit_stats(hitCounts.as<uint32_t>(), N, h));
        *out = r.kind == STAT_HIT_OVERFLOW ? (double)h[0] : (r.kind == STAT_HIT_MEAN ? (double)h[1] / (double)N : (r.kind == STAT_HIT_MAX ? (double)h[2] : (double)h[3]));
        return NRS_OK;
    }
    // bookkeeping at the end of a completed step (cell-table undo, buffer swaps)
    int end_of_step()
    {
        if (sparse_cell_table(P.numCells, n)) { // big, mostly empty table: undo only the touched cells
            if (!splitClearedCells)
                hipLaunchKernelGGL(k_clear_cells, dim3(nblocks(n)), dim3(BLOCK), 0, stream, sort.hash(), cellStart.as<uint32_t>(), (uint32_t)n);
            cellsClean = true;
        }
        // the integrated sorted arrays become the next step's input (replaces D2H + H2D)
        ++stepsDone;
        st.step_ended(fusedThisStep); // fused: A holds the new state in the slot order of sort.hash()
        if (!fusedThisStep) { // the fused kernel already wrote the new state into A
            std::swap(posA.p, posB.p);
            std::swap(velA.p, velB.p);
        }
        if (pressure_swaps(cfg.solver)) std::swap(presA.p, presB.p); // (PCISPH: the solve left its final pressures in presB, PBF its lambda, DFSPH K)
        ps.kv_swap(); // (DFSPH's Kv follows the particles)
        if (track.on) track.swap();
        return NRS_OK;
    }
    int step(int nsteps, int stop) override
    {
        if (ps.host_step()) return fail(NRS_E_STATE, "a host-driven IISPH step is in progress (nrs_iisph_finish first)");
        NRSCHK(validate("nrs_step"));
        if (midStep) return fail(NRS_E_STATE, "state is mid-update after nrs_step_partial; upload particles first");
        NRSCHK(stage_allowed(cfg.solver, stop));
        const bool sources = inflow.active(); // sinks, then emitters, at the top of every step; an enabled emitter steps from empty
        if (n == 0 && !(sources && inflow.emitter_enabled())) return NRS_OK;
        NRSCHK(ps.prepare(P, stream));
        for (int s = 0; s < nsteps; ++s) {
            if (sources) {
                NRSCHK(apply_inflow());
                if (n == 0) continue; // (still empty: nothing to step)
            }
            fusedThisStep = false;
            splitClearedCells = false;
            plan = plan_step(stop);
            NRSCHK(advance_bodies_and_rebuild());
            NRSCHK(stage_prefix(stop));
            if (stop && stop <= NRS_STAGE_REORDER) { midStep = true; break; }
            NRSCHK(with_walls([&](auto hasB) { return tail<hasB>(stop); }));
            HIPCHK(hipGetLastError());
            if (stop) { midStep = true; break; }
            NRSCHK(end_of_step());
        }
        HIPCHK(hipGetLastError());
        if (timer.used > 8192) NRSCHK(timer.collect(stream)); // bound the pool of pending event pairs
        return NRS_OK;
    }
    // the device-side guard (GridView::err) fired since the last check: report it, once
    int check_device_error()
    {
        uint32_t e = 0;
        HIPCHK(hipMemcpyAsync(&e, errWord.p, 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (!e) return NRS_OK;
        HIPCHK(hipMemsetAsync(errWord.p, 0, 4, stream));
        return fail(NRS_E_STATE, "device-side consistency check failed: a cell range lies outside the sorted particle array (the cell table was "
                                 "built from an inconsistent sort); the neighbour sweep skipped it, results of the last steps are invalid");
    }
    int sync() override
    {
        HIPCHK(hipStreamSynchronize(stream));
        return check_device_error();
    }
    // ---- asynchronous snapshots for a viewer (include/nereus_hip.h: nrs_snapshot_*) ---------------------------
    SnapshotRing snapshots;
    uint64_t stepsDone = 0;
    int snapshot_begin(int withVel) override
    {
        NRSCHK(validate("nrs_snapshot_begin"));
        if (midStep) return fail(NRS_E_STATE, "state is mid-update");
        NRSCHK(compact_holes());
        return snapshots.begin(posA.p, withVel ? velA.p : nullptr, sizeof(T4), cap, n, stepsDone, stream);
    }
    int snapshot_wait(int block, const void **pos4, const void **vel4, uint64_t *np, uint64_t *step) override
    {
        return snapshots.wait(block, pos4, vel4, np, step);
    }

    int download(void *pos4, void *vel4, void *pres) override
    {
        NRSCHK(validate("nrs_download"));
        NRSCHK(compact_holes());
        if (pos4) HIPCHK(hipMemcpyAsync(pos4, posA.p, sizeof(T4) * n, hipMemcpyDeviceToHost, stream));
        if (vel4) HIPCHK(hipMemcpyAsync(vel4, velA.p, sizeof(T4) * n, hipMemcpyDeviceToHost, stream));
        if (pres) HIPCHK(hipMemcpyAsync(pres, presA.p, sizeof(R) * n, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return check_device_error();
    }
    // which buffer an id means on this context, or its refusal: route_array (nrs_host_solver.h)
    int array(int which, void **dptr, uint64_t *bytes) override
    {
        if (which == NRS_ARR_POS || which == NRS_ARR_VEL) NRSCHK(compact_holes());
        ArrayRoute r;
        NRSCHK(route_array(which, ArrayRouteFacts{cfg.solver, midStep, bt.count() != 0, bt.has_bodies(), ps.pbfSt.vortValid, ps.akSt.normalsValid,
                                                  ps.dfSt.alphaValid, ps.dfSt.kvValid, ps.pciSt.xs}, r));
        const uint64_t count = (r.unit == UNIT_U32_CELLS) ? P.numCells : (r.unit == UNIT_VEC4_NB || r.unit == UNIT_U32_NB) ? bt.count() : n;
        const uint64_t elem = (r.unit == UNIT_VEC4_N || r.unit == UNIT_VEC4_NB) ? sizeof(T4) : r.unit == UNIT_SCALAR_N ? sizeof(R) : 4;
        *dptr = buf_ptr(r.buf);
        *bytes = (*dptr || which == NRS_ARR_B_BODY) ? elem * count : 0;
        return NRS_OK;
    }

    // ---- field sampling, surface extraction, diffuse particles (include/nereus_hip.h; DESIGN.md under these names) ---------------------------
    // The add-ons that only read the particle state have one owner: rd (nrs_readers.h) holds the sampler, the mesher and the diffuse set, launches,
    // copies out and names what their results hold.  The context counts what the sampler's cache rule depends on, checks its own state and says what
    // the fluid is now; every call below forwards.
    FluidReaders<R, KSET> rd;
    uint64_t particleGen = 0, gridGen = 0, boundaryGen = 0; // uploads / nrs_set_num_particles, grid changes, boundary sets / body assignments
    FluidNow<R> fluid_now() const
    {
        const SampleFacts facts{midStep, ps.host_step(), exch.on(), {P.gridSize[0], P.gridSize[1], P.gridSize[2]},
                                {(double)P.cellSize[0], (double)P.cellSize[1], (double)P.cellSize[2]}, (double)P.interactionRadius};
        return FluidNow<R>{P, posA.as<T4>(), velA.as<T4>(), n, SampleKey{stepsDone, particleGen, gridGen, boundaryGen}, facts,
                           bt.cell_start(), bt.cell_end(), bt.sorted(), bt.count(), stream};
    }
    int sample_points(const void *points4, uint64_t m, uint32_t fields) override
    {
        NRSCHK(validate("nrs_sample_*"));
        return rd.sample_points(fluid_now(), points4, m, fields);
    }
    int sample_lattice(const nrs_lattice *lattice, uint32_t fields) override { NRSCHK(validate("nrs_sample_*")); return rd.sample_lattice(fluid_now(), lattice, fields); }
    int sample_device_ptr(uint32_t field, void **dptr, uint64_t *bytes) override { return rd.sample_device_ptr(field, dptr, bytes); }
    int sample_result(uint32_t field, void *dst, uint64_t dstBytes, uint64_t *outBytes) override { return rd.sample_result(field, dst, dstBytes, outBytes, stream); }
    uint64_t sample_builds() override { return rd.sm.cache.builds; }
    int sample_release() override { return rd.release(rd.sm, stream); }
    int surface_extract(const nrs_lattice *lattice, double iso, uint32_t flags, uint64_t *vertices, uint64_t *triangles) override
    {
        NRSCHK(surface_check_call(iso, flags)); // (its refusals come before the state check's)
        NRSCHK(validate("nrs_sample_*"));
        return rd.surface_extract(fluid_now(), lattice, iso, flags, vertices, triangles);
    }
    int surface_device_ptr(uint32_t which, void **dptr, uint64_t *bytes) override { return rd.surface_device_ptr(which, dptr, bytes); }
    int surface_result(uint32_t which, void *dst, uint64_t dstBytes, uint64_t *outBytes) override { return rd.surface_result(which, dst, dstBytes, outBytes, stream); }
    int surface_release() override { return rd.release(rd.sf, stream); }
    int aniso_build(const nrs_aniso_config *cfg) override { NRSCHK(validate("nrs_sample_*")); return rd.aniso_build(fluid_now(), cfg); }
    int aniso_result(uint32_t which, void *dst, uint64_t dstBytes, uint64_t *outBytes) override { return rd.aniso_result(which, dst, dstBytes, outBytes, stream); }
    int aniso_device_ptr(uint32_t which, void **dptr, uint64_t *bytes) override { return rd.aniso_device_ptr(which, dptr, bytes); }
    int aniso_release() override { return rd.release(rd.an, stream); }
    int surface_extract_aniso(const nrs_lattice *lattice, double iso, uint32_t flags, const nrs_aniso_config *cfg, uint64_t *vertices,
                              uint64_t *triangles) override
    {
        NRSCHK(aniso_check_extract(iso, flags)); // (its refusals come before the state check's)
        NRSCHK(validate("nrs_sample_*"));
        return rd.surface_extract_aniso(fluid_now(), lattice, iso, flags, cfg, vertices, triangles);
    }
    int diffuse_configure(const nrs_diffuse_config *c) override { NRSCHK(validate("nrs_diffuse_configure")); return rd.diffuse_configure(fluid_now(), c); }
    int diffuse_step(double dt) override { NRSCHK(validate("nrs_diffuse_step")); return rd.diffuse_step(fluid_now(), dt); }
    int diffuse_count(uint64_t *alive, uint64_t *byKind, uint64_t *dropped) override
    {
        NRSCHK(validate("nrs_diffuse_count"));
        return rd.diffuse_count(stream, alive, byKind, dropped);
    }
    int diffuse_device_ptr(uint32_t which, void **dptr, uint64_t *bytes) override { return rd.diffuse_device_ptr(which, dptr, bytes, stream); }
    int diffuse_result(uint32_t which, void *dst, uint64_t dstBytes, uint64_t *outBytes) override { return rd.diffuse_result(which, dst, dstBytes, outBytes, stream); }
    int diffuse_upload(const void *pos4, const void *vel4, uint64_t count) override
    {
        NRSCHK(validate("nrs_diffuse_upload"));
        return rd.diffuse_upload(fluid_now(), pos4, vel4, count);
    }
    int diffuse_release() override { return rd.release(rd.df, stream); }

    // ---- sources and sinks (include/nereus_hip.h; DESIGN.md "Sources and sinks") ----------------------------------------------------------------
    // The slots, the sink configuration, the counts and the cull's buffers are inflow's (nrs_inflow.h); the arrays, the count and the state
    // transition are the context's.  Emission writes behind the living particles of the A arrays; a cull that removes something moves
    // A -> B and swaps, as end_of_step does.  Both leave the state nrs_upload_particles leaves (particles_changed).
    InflowSystem inflow;
    int inflow_begin(const char *where, bool driven) const
    {
        NRSCHK(validate(where));
        return inflow_refusal(exch.on(), midStep, ps.host_step(), driven);
    }
    void particles_changed()
    {
        ++particleGen;
        st.to_fresh();
    }
    // where the particles of emit value `slot` (-1: nrs_emit_block) go; tracking: their ids start at firstId
    EmitOut<R> emit_out(int32_t slot, uint32_t firstId)
    {
        EmitOut<R> O{};
        O.pos = posA.as<T4>(); O.vel = velA.as<T4>(); O.pres = presA.as<R>(); O.kv = ps.kv_current();
        O.first = (uint32_t)n;
        if (track.on) {
            const TrackView<R> v = track.template cur<R>();
            const double *a = track.emit_value(slot);
            O.id = v.id; O.birth = v.birth; O.rec = v.rec;
            O.firstId = firstId; O.birthNow = track_birth(stepsDone);
            O.recValue.x = (R)a[0]; O.recValue.y = (R)a[1]; O.recValue.z = (R)a[2]; O.recValue.w = (R)a[3];
        }
        return O;
    }
    int emitter_set(uint32_t slot, const nrs_emitter *e) override
    {
        NRSCHK(inflow_check_slot(slot));
        EmitterSlot fresh;
        if (e) NRSCHK(inflow_check_emitter(e, (double)PU.particleMass, (double)PU.restDensity, fresh));
        NRSCHK(inflow_begin("nrs_emitter_set", false));
        inflow.slots[slot] = std::move(fresh);
        return NRS_OK;
    }
    int emitter_get(uint32_t slot, nrs_emitter *e, uint64_t *emitted, uint64_t *dropped) override
    {
        NRSCHK(inflow_check_slot(slot));
        const EmitterSlot &sl = inflow.slots[slot];
        if (e) *e = sl.e;
        if (emitted) *emitted = sl.emitted;
        if (dropped) *dropped = sl.dropped;
        return NRS_OK;
    }
    int emit_block(const nrs_lattice *lattice, const double *vel, uint64_t *added) override
    {
        if (added) *added = 0;
        NRSCHK(validate("nrs_emit_block"));
        if (exch.on()) return inflow_refusal(true, false, false, true);
        uint64_t m = 0;
        NRSCHK(inflow_check_block(lattice, vel, n, cap, &m));
        NRSCHK(inflow_refusal(false, midStep, ps.host_step(), true));
        uint32_t firstId = 0;
        if (track.on) NRSCHK(track.ids.reserve(m, &firstId));
        NRSCHK(inflow.template emit_block<R>(lattice_from(*lattice), vel, (uint32_t)m, emit_out(-1, firstId), stream));
        n += m;
        particles_changed();
        if (added) *added = m;
        return NRS_OK;
    }
    // nrs_emit_mesh: the selection runs on the device (MeshSampler, nrs_mesh.h: at most capacity - n node indices are kept), the count is
    // read back (the one wait), then the append; the sampler's buffers go before the call returns
    MeshSampler meshSampler;
    int emit_mesh(const nrs_mesh *mesh, const nrs_lattice *lattice, const nrs_mesh_rule *rule, const double *vel, uint64_t *added) override
    {
        if (added) *added = 0;
        NRSCHK(validate("nrs_emit_mesh"));
        if (exch.on()) return inflow_refusal(true, false, false, true);
        uint64_t nodes = 0;
        NRSCHK(inflow_check_sites(lattice, vel, &nodes));
        NRSCHK(mesh_check_mesh(mesh));
        NRSCHK(mesh_check_rule(rule));
        if (rule->flags & NRS_MESH_SNAP) return mesh_refuse_snap();
        NRSCHK(inflow_refusal(false, midStep, ps.host_step(), true));
        const int rc = emit_mesh_checked(*mesh, lattice_from(*lattice), nodes, *rule, vel, added);
        (void)hipStreamSynchronize(stream); // (the append reads the selection)
        meshSampler.release();
        return rc;
    }
    int emit_mesh_checked(const nrs_mesh &mesh, const Lattice &L, uint64_t nodes, const nrs_mesh_rule &rule, const double *vel, uint64_t *added)
    {
        const uint64_t room = cap - n;
        uint64_t m = 0;
        NRSCHK(meshSampler.upload(mesh, stream));
        NRSCHK(meshSampler.select(L, nodes, rule, room, stream, &m));
        if (m > room) return fail(NRS_E_CAPACITY, "emit mesh: more nodes selected than capacity - n");
        if (!m) return NRS_OK;
        uint32_t firstId = 0;
        if (track.on) NRSCHK(track.ids.reserve(m, &firstId));
        NRSCHK(inflow.template emit_sites<R>(L, meshSampler.selected(), vel, (uint32_t)m, emit_out(-1, firstId), stream));
        n += m;
        particles_changed();
        if (added) *added = m;
        return NRS_OK;
    }
    int sinks_set(const nrs_sink_config *c) override
    {
        if (c) NRSCHK(inflow_check_sinks(c));
        NRSCHK(inflow_begin("nrs_sinks_set", false));
        inflow.set_sinks(c);
        return NRS_OK;
    }
    int sinks_count(uint64_t *removedTotal, uint64_t *culls) override
    {
        if (removedTotal) *removedTotal = inflow.removedTotal;
        if (culls) *culls = inflow.culls;
        return NRS_OK;
    }
    // one cull with the current sinks: count, scan, read the survivor count back (the wait); only when something goes: compact and swap
    // (in two halves: between them the top of a tracked step learns how much room its emitters get, and may still refuse)
    CullBounds<R> cull_bounds() const { return inflow_bounds<R>(inflow.haveSinks ? &inflow.sinks : nullptr, PU.worldOrigin, PU.gridSize, PU.cellSize); }
    int cull_count(uint32_t *keep)
    {
        *keep = (uint32_t)n;
        if (!n) return NRS_OK;
        NRSCHK(inflow.template count<R>(posA.as<T4>(), cull_bounds(), (uint32_t)n, stream, keep));
        if (*keep > n) return fail(NRS_E_STATE, "cull: more survivors than particles");
        return NRS_OK;
    }
    int cull_finish(uint32_t keep, uint64_t *removed)
    {
        *removed = 0;
        const uint32_t N = (uint32_t)n;
        if (keep < N) {
            CullArrays<R> A{posA.as<T4>(), velA.as<T4>(), presA.as<R>(), ps.kv_current(), posB.as<T4>(), velB.as<T4>(), presB.as<R>(), ps.kv_other()};
            if (track.on) {
                const TrackView<R> from = track.template cur<R>(), to = track.template other<R>();
                A.id = from.id; A.birth = from.birth; A.rec = from.rec;
                A.idTo = to.id; A.birthTo = to.birth; A.recTo = to.rec;
            }
            NRSCHK(inflow.template compact<R>(A, cull_bounds(), N, stream));
            std::swap(posA.p, posB.p);
            std::swap(velA.p, velB.p);
            std::swap(presA.p, presB.p);
            ps.kv_swap();
            if (track.on) track.swap();
            *removed = N - keep;
            n = keep;
            particles_changed();
        }
        inflow.culled(*removed);
        return NRS_OK;
    }
    int cull_now(uint64_t *removed)
    {
        uint32_t keep = 0;
        *removed = 0;
        NRSCHK(cull_count(&keep));
        return cull_finish(keep, removed);
    }
    int cull(uint64_t *removed) override
    {
        uint64_t r = 0;
        if (removed) *removed = 0;
        NRSCHK(inflow_begin("nrs_cull", true));
        NRSCHK(cull_now(&r));
        if (removed) *removed = r;
        return NRS_OK;
    }
    // the top of a step (step(), nrs_iisph_predict): the sinks, then the emitters' layers of this step, slots ascending
    int apply_inflow()
    {
        const bool due = inflow.cull_due();
        uint32_t keep = (uint32_t)n;
        if (due) NRSCHK(cull_count(&keep));
        if (track.on && track_ids_of_step(keep) != NRS_OK) { // refused before anything moved: this step does not count
            inflow.step_not_taken();
            return NRS_E_CAPACITY;
        }
        if (due) {
            uint64_t r = 0;
            NRSCHK(cull_finish(keep, &r));
        }
        bool any = false;
        std::vector<double> offsets;
        for (uint32_t si = 0; si < (uint32_t)NRS_MAX_EMITTERS; ++si) {
            uint64_t room = cap - n;
            const uint64_t before = room;
            offsets.clear();
            inflow_schedule(inflow.slots[si], (double)PU.timestep, room, offsets);
            if (offsets.empty()) continue;
            uint32_t firstId = 0;
            if (track.on) NRSCHK(track.ids.reserve(before - room, &firstId)); // (fits: track_ids_of_step)
            NRSCHK(inflow.template emit<R>(si, offsets, emit_out((int32_t)si, firstId), stream));
            n += before - room;
            any = true;
        }
        if (any) particles_changed();
        return NRS_OK;
    }
    // the ids this step's layers need, with `living` particles behind the cull: the schedule counted without touching the slots (inflow_schedule_count); NRS_E_CAPACITY when
    // they pass the last id, with nothing changed
    int track_ids_of_step(uint32_t living) const
    {
        if (!inflow.emitter_enabled()) return NRS_OK;
        uint64_t room = cap - living, need = 0;
        for (const EmitterSlot &sl : inflow.slots) need += inflow_schedule_count(sl, (double)PU.timestep, room);
        return track_ids_fit(track.ids.next, need);
    }

    // ---- particle identity and attributes (include/nereus_hip.h; DESIGN.md "Particle identity and attributes") ----------------------------------
    // The tracked arrays, the id counter and the emit values are track's (nrs_track.h).  They follow the particle arrays: gathered behind a
    // step's reorder (stage_prefix), swapped where those swap (end_of_step, cull_finish), written by emission, filled for the slots an
    // upload or a count change makes new.  With tracking never enabled nothing here runs.
    TrackSystem track;
    TrackFacts track_facts() const { return TrackFacts{track.on, track.flags, midStep, ps.host_step()}; }
    // the slots f of the current order are new particles: fresh ids, born now, the emit value of slot -1
    int track_new_slots(const TrackFresh &f)
    {
        uint32_t firstId = 0;
        NRSCHK(track.ids.reserve(f.count, &firstId));
        return track.template fill<R>(f.first, f.count, firstId, track_birth(stepsDone), track.emit_value(-1), stream);
    }
    int track_enable(uint32_t flags) override
    {
        NRSCHK(track_check_flags(flags));
        if (exch.on()) return track_refuse_slab();
        NRSCHK(refuse_mid_iisph("nrs_track_enable"));
        NRSCHK(validate("nrs_track_enable"));
        return track.template enable<R>(flags, cap, n, stream);
    }
    int track_disable() override { return track.disable(stream); }
    int track_info(int *on, uint32_t *flags, uint64_t *nextId) override
    {
        if (on) *on = track.on ? 1 : 0;
        if (flags) *flags = track.flags;
        if (nextId) *nextId = track.ids.next;
        return NRS_OK;
    }
    int track_upload(uint32_t which, const void *src, uint64_t first, uint64_t count) override
    {
        NRSCHK(track_refusal(track_facts(), false, false));
        NRSCHK(refuse_mid_iisph("nrs_track_upload"));
        NRSCHK(track_check_upload(which, track.flags, src, first, count, n));
        uint64_t next = track.ids.next;
        if (which == NRS_TRACK_ID) NRSCHK(track_ids_uploaded((const uint32_t *)src, count, next, &next));
        NRSCHK(track.template upload<R>(which, src, first, count, stream));
        track.ids.next = next;
        return NRS_OK;
    }
    int track_device_ptr(uint32_t which, void **dptr, uint64_t *bytes) override
    {
        NRSCHK(track_refusal(track_facts(), false, true));
        NRSCHK(track_route_result(which, track.flags, track.haveLocate, n, track.located, FluidReaders<R, KSET>::PRECISION, bytes));
        *dptr = *bytes ? track.result(which) : nullptr;
        return NRS_OK;
    }
    int track_result(uint32_t which, void *dst, uint64_t dstBytes, uint64_t *outBytes) override
    {
        void *p = nullptr;
        uint64_t sz = 0;
        NRSCHK(track_device_ptr(which, &p, &sz));
        return FluidReaders<R, KSET>::copy_out(dst, dstBytes, p, sz, outBytes, stream);
    }
    int track_emit_value(int32_t slot, const double *a) override
    {
        NRSCHK(track_refusal(track_facts(), true, false));
        NRSCHK(track_check_emit_value(slot, a));
        std::memcpy(track.emitValue[slot + 1], a, 4 * sizeof(double));
        return NRS_OK;
    }
    int track_locate(uint64_t firstId, uint64_t count) override
    {
        NRSCHK(track_refusal(track_facts(), false, true));
        NRSCHK(track_check_locate(firstId, count));
        return track.locate(firstId, count, n, stream);
    }
    // on the sampler's particle grid (its refusals, its cache rule, nrs_sample_builds), as the diffuse particles read the fluid
    int track_diffuse(const double *kappa, double dt) override
    {
        NRSCHK(track_refusal(track_facts(), true, true));
        NRSCHK(track_check_diffuse(kappa, dt));
        NRSCHK(validate("nrs_track_diffuse"));
        const FluidNow<R> f = fluid_now();
        NRSCHK(sample_refusal(f.facts));
        const bool walls = bt.count() != 0;
        GridView<R> G;
        NRSCHK(rd.grid(f, walls, G));
        return track.template diffuse<R, KSET>(P, G, walls, rd.sm.template sorted_pos<T4>(), rd.sm.template sorted_vel<T4>(), rd.sm.sorted_index(),
                                               rd.sm.sorted_count(), kappa, dt == 0.0 ? (double)P.timestep : dt, stream);
    }
};

template <typename R, int KSET> CtxBase *make_ctx2(bool surf)
{
    if (surf) return new Ctx<R, KSET, true>();
    return new Ctx<R, KSET, false>();
}

} // namespace nrs
