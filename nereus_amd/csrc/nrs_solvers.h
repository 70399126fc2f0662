// nrs_solvers.h — the owner of the four pressure solvers behind the SESPH step (DESIGN.md "IISPH", "PCISPH", "PBF", "DFSPH", "Akinci"):
// their buffers (BufName, nrs_host_solver.h), their settings, derived constants and what the last step left (one state struct per
// solver), the launches of their chains and the reductions of their exit tests.  It depends on the precision, the kernel set and the
// surface term; the context (nrs_ctx_impl.h) holds one, forwards the configure calls, and hands every chain one SolverStep: what the
// step is now.  What a chain needs of the context beyond that is one callable, the step's last launch (Ctx::launch_last); this step's
// wall list is built by the context before the chain starts.  The particle arrays stay the context's: the owner sees the sorted ones
// through SortedArrays, and DFSPH's Kv pair, which follows the particles, through the kv_* operations.
// Here once: whether a neighbour launch takes the reference-order kernel or the list kernel (ref_or_lists), with or without wall
// workgroups (gather); the sorted-array arguments of a kernel (SortedArrays); the reductions (Reductions, which the context uses too).
#pragma once
#include <tuple>
#include <type_traits>

#include "nrs_ctx_base.h"
#include "nrs_host_plan.h"
#include "nrs_host_profile.h"
#include "nrs_host_solver.h"

#include "nrs_kernels_ref.h"
#include "nrs_kernels_tiled.h"
#include "nrs_kernels_iisph.h"
#include "nrs_kernels_pcisph.h"
#include "nrs_kernels_pbf.h"
#include "nrs_kernels_dfsph.h"
#include "nrs_kernels_akinci.h"
#include "nrs_viscosity.h"

namespace nrs {

// ---- reductions over a per-particle array, deterministic: per-block partials on the device, combined in a fixed order -------------------
template <typename R> struct Reductions {
    typedef typename Vec4T<R>::type T4;
    int init(hipStream_t s)
    {
        stream = s;
        NRSCHK(partial.alloc(sizeof(double) * 1024));
        return out.alloc(2 * sizeof(double));
    }
    // the landing of a one-block kernel's doubles (the prototype sums, W_q), and `count` of them read back, waited for
    double *scratch() const { return partial.as<double>(); }
    int read_scratch(double *o, int count)
    {
        HIPCHK(hipMemcpyAsync(o, partial.p, count * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return NRS_OK;
    }
    int sum(const R *a, uint32_t N, double *o)
    {
        sum_to(a, N, out.as<double>());
        HIPCHK(hipMemcpyAsync(o, out.p, sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return NRS_OK;
    }
    // the sum left in a device slot, nothing read back and nothing waited for (sum's two launches; the CG sums of nrs_viscosity.h)
    void sum_to(const R *a, uint32_t N, double *slot)
    {
        const uint32_t nbk = std::min<uint32_t>(1024u, nblocks(N));
        hipLaunchKernelGGL((k_sum_partial<R>), dim3(nbk), dim3(BLOCK), 0, stream, a, scratch(), N);
        hipLaunchKernelGGL(k_sum_final, dim3(1), dim3(BLOCK), 0, stream, scratch(), slot, nbk);
    }
    // the sum, and how many of the N particles a slab rank owns (ownedPos: their sorted positions; null: no count is formed)
    int sum_and_count(const R *a, uint32_t N, const T4 *ownedPos, double *o, uint64_t *owned)
    {
        const uint32_t nbk = std::min<uint32_t>(1024u, nblocks(N));
        unsigned long long *cnt = (unsigned long long *)out.p; // out: [double sum][u64 count]
        HIPCHK(hipMemsetAsync(out.p, 0, 16, stream));
        hipLaunchKernelGGL((k_sum_partial<R>), dim3(nbk), dim3(BLOCK), 0, stream, a, scratch(), N, ownedPos, cnt + 1);
        hipLaunchKernelGGL(k_sum_final, dim3(1), dim3(BLOCK), 0, stream, scratch(), out.as<double>(), nbk);
        double h[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(h, out.p, 16, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        unsigned long long c;
        std::memcpy(&c, &h[1], 8);
        *o = h[0];
        *owned = (uint64_t)c;
        return NRS_OK;
    }
    // max over an SReal array (VEC: of |v| over a vec4 array): per-block maxima on the device, their max on the host
    template <bool VEC> int max_of(const void *a, uint32_t N, double *o)
    {
        const uint32_t nbk = std::min<uint32_t>(1024u, nblocks(N));
        hipLaunchKernelGGL((k_max_partial<R, VEC>), dim3(nbk), dim3(BLOCK), 0, stream, a, scratch(), N);
        std::vector<double> h(nbk);
        HIPCHK(hipMemcpyAsync(h.data(), partial.p, sizeof(double) * nbk, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        double m = h[0];
        for (uint32_t i = 1; i < nbk; ++i) m = std::max(m, h[i]);
        *o = m;
        return NRS_OK;
    }
    // k_hit_stats over the hit counts of N slots: overflowed lists, the sum of the lengths, the longest, the unstaged hits
    int hit_stats(const uint32_t *counts, uint32_t N, unsigned long long h[4])
    {
        HIPCHK(hipMemsetAsync(partial.p, 0, 4 * sizeof(unsigned long long), stream));
        hipLaunchKernelGGL(k_hit_stats, dim3(std::min<uint32_t>(1024u, nblocks(N))), dim3(BLOCK), 0, stream, counts, (unsigned long long *)partial.p, N);
        HIPCHK(hipMemcpyAsync(h, partial.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return NRS_OK;
    }

private:
    hipStream_t stream = nullptr;
    DevBuf partial, out;
};

// ---- what a step is now, as the context tells a solver chain -------------------------------------------------------------------------------
// The sorted particle arrays of the step.  Every kernel takes a subset of them in this order, then the count: the four subsets are
// spelled here and nowhere else.
template <typename R> struct SortedArrays {
    typedef typename Vec4T<R>::type T4;
    T4 *pos, *vel;
    R *dens, *pres;
    uint32_t N;
    std::tuple<T4 *, uint32_t> p() const { return {pos, N}; }
    std::tuple<T4 *, R *, uint32_t> pd() const { return {pos, dens, N}; }
    std::tuple<T4 *, R *, R *, uint32_t> pdp() const { return {pos, dens, pres, N}; }
    std::tuple<T4 *, T4 *, R *, R *, uint32_t> pvdp() const { return {pos, vel, dens, pres, N}; }
};
template <typename R> struct SolverStep {
    typedef typename Vec4T<R>::type T4;
    const Params<R> &P;     // the kernels' parameters
    StepPlan plan;          // which kernels the step launches (nrs_host_plan.h)
    StepPlan repeat;        // IISPH: the plan of the repeat in reference order of a diverged list-driven step (plan.watch)
    GridView<R> G;
    CutThresholds thr;
    HitBuffer hb;           // the hit lists the density scan builds and the gathers behind it consume
    WallList walls;         // this step's wall list, built before the chain starts (plan.walls)
    SortedArrays<R> sorted; // posB, velB, dens, presB and the particle count
    const R *presA;         // IISPH's repeat gathers the warm-start pressures again: the unsorted ones ...
    const uint32_t *sortIndex; // ... and the sorted values
    uint32_t *nonFinite;    // IISPH: the word a list kernel raises when a gathered value is not finite (plan.watch)
    bool slab;              // a slab run is on ...
    int slabMaxIters;       // ... whose halo width supports this many solver iterations
    bool movingWalls;       // this step rebuilt the boundary tables at new poses ...
    const T4 *wallVel;      // ... and these are the wall particles' velocities, in sorted order
    uint32_t maxIters;      // nrs_set_max_iterations (0: the solver's default)
    uint32_t *iters;        // where the iteration count of the step's solve goes (nrs_last_iterations)
    StageTimer *timer;      // profiling (nrs_host_profile.h)
    uint32_t profMask;
    hipStream_t stream;
};

template <typename R, int KSET, bool SURF> struct PressureSolvers {
    typedef typename Vec4T<R>::type T4;
    typedef SolverStep<R> Step;
    PressureSolvers(Reductions<R> &r, ViscositySolver<R> &v) : red(r), visc(v) {}

    // per solver: settings, derived constants, what the last step left (nrs_host_solver.h).  PBF shares pciSt.xs and pciSt.lastErr.
    PciState<R> pciSt;   // nrs_kernels_pcisph.h
    PbfState<R> pbfSt;   // nrs_kernels_pbf.h
    DfsphState<R> dfSt;  // nrs_kernels_dfsph.h; DESIGN.md "DFSPH"
    AkinciState akSt;    // nrs_kernels_akinci.h; PCISPH, PBF, DFSPH
    uint64_t iisphRestarts = 0; // list-driven IISPH steps repeated in reference order

    // ---- buffers ----------------------------------------------------------------------------------------------------------------------
    // what solver_buffers lists for the solver, allocated and zero-filled in the table's order
    int init(int solver_, uint64_t cap_, hipStream_t stream)
    {
        solver = solver_;
        cap = cap_;
        const size_t v = sizeof(T4) * cap, s = sizeof(R) * cap, u = 4 * cap;
        const SolverBufferList own = solver_buffers(solver);
        for (const SolverBuffer &b : own) {
            size_t bytes = 0;
            switch (b.unit) { // (the table's contract: per-particle units, sized by the capacity)
            case UNIT_VEC4_N: bytes = v; break;
            case UNIT_SCALAR_N: bytes = s; break;
            case UNIT_U32_N: bytes = u; break;
            case UNIT_U32_CELLS: case UNIT_VEC4_NB: case UNIT_U32_NB: return fail(NRS_E_STATE, "solver_buffers lists a buffer that is not per particle");
            }
            NRSCHK(devbuf(b.buf)->alloc(bytes));
        }
        for (const SolverBuffer &b : own)
            if (b.zero) HIPCHK(hipMemsetAsync(devbuf(b.buf)->p, 0, devbuf(b.buf)->bytes, stream));
        return NRS_OK;
    }
    // the solvers' BufNames: where the array lives and its allocated bytes; false for any other name
    bool buffer(BufName b, void **p, size_t *bytes)
    {
        const DevBuf *d = devbuf(b);
        if (!d) return false;
        *p = d->p;
        *bytes = d->bytes;
        return true;
    }
    uint32_t *inverse_slots() const { return inv.as<uint32_t>(); } // IISPH: written by the reorder kernels

    // ---- DFSPH's Kv pair follows the particles (A: slot order of the current arrays, B: sorted); null, or nothing done, on another solver ----
    bool dfsph() const { return solver == NRS_SOLVER_DFSPH; }
    R *kv_current() const { return dfsph() ? dfKvA.as<R>() : (R *)nullptr; }
    R *kv_other() const { return dfsph() ? dfKvB.as<R>() : (R *)nullptr; }
    void kv_swap() { if (dfsph()) std::swap(dfKvA.p, dfKvB.p); }
    int kv_zero(uint64_t first, uint64_t count, hipStream_t stream) // (uploaded particles: Kv restarts at zero; K is the pressure)
    {
        if (dfsph()) HIPCHK(hipMemsetAsync(dfKvA.as<R>() + first, 0, sizeof(R) * count, stream));
        return NRS_OK;
    }
    void kv_gather(const uint32_t *index, uint32_t N, hipStream_t stream) // Kv_prev into sorted order: a warm-start input of the step
    {
        hipLaunchKernelGGL((k_gather_scalar<R>), dim3(nblocks(N)), dim3(BLOCK), 0, stream, dfKvA.as<R>(), index, dfKvB.as<R>(), N);
        dfSt.kvValid = true;
    }

    // ---- settings and derived constants -------------------------------------------------------------------------------------------------
    void params_changed(const StaleConstants &stale)
    {
        pciSt.params_changed(stale);
        pbfSt.params_changed(stale);
        dfSt.params_changed(stale);
    }
    int pcisph_configure(double eta, uint32_t minIters, double spacing, double delta)
    {
        if (solver != NRS_SOLVER_PCISPH) return fail(NRS_E_STATE, "nrs_pcisph_configure on a context that is not PCISPH");
        NRSCHK(pciSt.s.set(eta, minIters, spacing, delta));
        pciSt.settings_changed();
        return NRS_OK;
    }
    int pbf_configure(double eta, uint32_t minIters, double relaxation, double xsph)
    {
        if (solver != NRS_SOLVER_PBF) return fail(NRS_E_STATE, "nrs_pbf_configure on a context that is not PBF");
        NRSCHK(pbfSt.s.set(eta, minIters, relaxation, xsph));
        pbfSt.settings_changed();
        return NRS_OK;
    }
    int pbf_set_tensile(const Params<R> &P, double k, double dq, hipStream_t stream)
    {
        if (solver != NRS_SOLVER_PBF) return fail(NRS_E_STATE, "nrs_pbf_set_tensile on a context that is not PBF");
        PbfSettings t = pbfSt.s;
        NRSCHK(t.set_tensile(k, dq));
        R wq;
        NRSCHK(pbf_eval_wq(P, dq, &wq, stream));
        pbfSt.s = t;
        pbfSt.set_wq(wq);
        return NRS_OK;
    }
    int pbf_set_vorticity(double epsV)
    {
        if (solver != NRS_SOLVER_PBF) return fail(NRS_E_STATE, "nrs_pbf_set_vorticity on a context that is not PBF");
        PbfSettings t = pbfSt.s;
        NRSCHK(t.set_vorticity(epsV));
        if (epsV > 0.0) NRSCHK(pbfVort.alloc(sizeof(T4) * cap));
        pbfSt.s = t;
        return NRS_OK;
    }
    int dfsph_configure(double eta, uint32_t minIters, double etaV, uint32_t minItersV, int warm)
    {
        if (!dfsph()) return fail(NRS_E_STATE, "nrs_dfsph_configure on a context that is not DFSPH");
        NRSCHK(dfSt.s.set(eta, minIters, etaV, minItersV, warm));
        return NRS_OK;
    }
    int dfsph_set_viscosity(double nu, double nuB, double tol, uint32_t minIters, uint32_t maxIters, bool movingBodies)
    {
        if (!dfsph()) return fail(NRS_E_STATE, "nrs_dfsph_set_viscosity on a context that is not DFSPH");
        return visc.configure(cap, nu, nuB, tol, minIters, maxIters, movingBodies);
    }
    int set_surface_akinci(double gamma, double beta)
    {
        if (solver != NRS_SOLVER_PCISPH && solver != NRS_SOLVER_PBF && !dfsph())
            return fail(NRS_E_STATE, "nrs_set_surface_akinci on a context that is not PCISPH, PBF or DFSPH");
        AkinciSettings a;
        NRSCHK(a.set(gamma, beta));
        if (gamma > 0.0) NRSCHK(akNormals.alloc(sizeof(T4) * cap));
        akSt.s = a;
        return NRS_OK;
    }
    // the solver's derived constant(s), each once per change of the parameters or settings it depends on; before the first step of a call.
    // P: the kernels' parameters, whose time step, mass, rest density and radius are the caller's (window_params changes the grid alone).
    int prepare(const Params<R> &P, hipStream_t stream)
    {
        if (solver == NRS_SOLVER_PCISPH) return pcisph_prepare(P, stream);
        if (solver == NRS_SOLVER_PBF) return pbf_prepare(P, stream);
        if (dfsph()) return dfsph_prepare(P, stream);
        return NRS_OK;
    }

    // ---- statistics on the solvers' buffers (route_stat, nrs_host_solver.h) -----------------------------------------------------------------
    // PBF, fixed-count solve: the max e of the last solve, still pending, into lastErr
    int form_pending_max()
    {
        NRSCHK(red.template max_of<false>(pciErr.p, pbfSt.errPending, &pciSt.lastErr));
        pbfSt.errPending = 0;
        return NRS_OK;
    }
    // DFSPH: max or average of the `count` e_i the last iteration of the density (pciErr) or divergence (dfErrV) solve left
    int dfsph_error(bool divergence, bool average, uint32_t count, double *out)
    {
        const void *e = divergence ? dfErrV.p : pciErr.p;
        if (!average) return red.template max_of<false>(e, count, out);
        double acc = 0.0;
        NRSCHK(red.sum((const R *)e, count, &acc));
        *out = acc / (double)count;
        return NRS_OK;
    }

    // ---- the chains: everything behind the reorder of a step that is not SESPH ----------------------------------------------------------------
    // last(plan, launch): the context's launch_last — the step's last launch, which also leaves the next step's sort keys
    template <bool HAS_B, typename Last> int tail(const Step &s, int stop, Last &&last)
    {
        switch (solver) {
        case NRS_SOLVER_IISPH: return iisph_tail<HAS_B>(s, stop, last);
        case NRS_SOLVER_PCISPH: return pcisph_tail<HAS_B>(s, stop, last);
        case NRS_SOLVER_PBF: return pbf_tail<HAS_B>(s, stop, last);
        case NRS_SOLVER_DFSPH: return dfsph_tail<HAS_B>(s, stop, last);
        default: return fail(NRS_E_STATE, "not a context of a pressure solver");
        }
    }
    // the host-driven IISPH step (multi-GPU: the loop exit needs the average over ALL ranks): nrs_iisph_predict / _iterate / _finish
    bool host_step() const { return iisphPhase != 0; } // predicted: iterations may follow
    void abandon_host_step() { iisphPhase = 0; iisphIter = 0; }
    void host_step_ended() { iisphPhase = 0; }
    template <bool HAS_B> int host_predict(const Step &s)
    {
        NRSCHK(iisph_predict<HAS_B>(s, 0));
        iisphPhase = 1;
        return NRS_OK;
    }
    // one iteration + the density-error sum over the particles this rank owns
    template <bool HAS_B> int host_iterate(const Step &s, double *sum, uint64_t *count)
    {
        if (s.slab && (int)iisphIter >= s.slabMaxIters)
            return fail(NRS_E_STATE, "IISPH slab run: more solver iterations than the halo width supports (halo >= 2 * iterations + 4 cells)");
        NRSCHK(iisph_iteration<HAS_B>(s));
        double h = 0.0;
        uint64_t c = 0;
        NRSCHK(red.sum_and_count(densCorr.as<R>(), s.sorted.N, s.slab ? s.sorted.pos : (const T4 *)nullptr, &h, &c));
        if (sum) *sum = h;
        if (count) *count = s.slab ? c : (uint64_t)s.sorted.N;
        *s.iters = iisphIter;
        return NRS_OK;
    }
    template <bool HAS_B, typename Last> int host_finish(const Step &s, Last &&last)
    {
        if (iisphIter == 0) return fail(NRS_E_STATE, "nrs_iisph_iterate at least once before nrs_iisph_finish");
        return iisph_finish<HAS_B>(s, 0, last);
    }

private:
    Reductions<R> &red;
    ViscositySolver<R> &visc; // DFSPH's implicit viscosity solve (nrs_viscosity.h): the context's, run behind the advection launch
    int solver = NRS_SOLVER_SESPH;
    uint64_t cap = 0;
    // the solvers' buffers (BufName, nrs_host_solver.h: which solver allocates which, and what the shared ones hold on each)
    DevBuf inv, densAdv, densCorr, P_l, P_l2, aii, velAdv, forcesAdv, forcesP, diiF, diiB, sumDij, diiSum;
    DevBuf posPred, posPred2, pciErr;
    DevBuf dfAlpha, dfKvA, dfKvB, dfErrV;
    DevBuf pbfVort, akNormals; // allocated when confinement is first enabled / gamma is first set above 0
    uint32_t iisphIter = 0;     // solver iterations done in the current step
    int iisphPhase = 0;         // 0 idle, 1 predicted (iterations may follow)
    bool iisphDiverged = false; // the last pass of the chain raised Step::nonFinite

    DevBuf *devbuf(BufName b)
    {
        switch (b) {
        case BUF_INV: return &inv; case BUF_DENS_ADV: return &densAdv; case BUF_P_L2: return &P_l2; case BUF_AII: return &aii;
        case BUF_DII_F: return &diiF; case BUF_DII_B: return &diiB; case BUF_SUM_DIJ: return &sumDij; case BUF_DII_SUM: return &diiSum;
        case BUF_VEL_ADV: return &velAdv; case BUF_FORCES_ADV: return &forcesAdv; case BUF_FORCES_P: return &forcesP;
        case BUF_DENS_CORR: return &densCorr; case BUF_P_L: return &P_l; case BUF_POS_PRED: return &posPred; case BUF_POS_PRED2: return &posPred2;
        case BUF_PCI_ERR: return &pciErr; case BUF_DF_ALPHA: return &dfAlpha; case BUF_DF_KV_A: return &dfKvA; case BUF_DF_KV_B: return &dfKvB;
        case BUF_DF_ERR_V: return &dfErrV; case BUF_PBF_VORT: return &pbfVort; case BUF_AK_NORMALS: return &akNormals;
        // no default: -Wswitch names a BufName that is missing here.  The particle arrays, the cell table and the sorted keys / values
        // are the context's (Ctx::buf_ptr), the boundary's arrays live in its BoundaryTables.
        case BUF_NONE: case BUF_POS_A: case BUF_POS_B: case BUF_VEL_A: case BUF_VEL_B: case BUF_PRES_A: case BUF_PRES_B: case BUF_DENS: case BUF_FORCES:
        case BUF_HASH_CUR: case BUF_INDEX_CUR: case BUF_CELL_START: case BUF_CELL_END: case BUF_COUNT: break;
        case BUF_B_HASH_CUR: case BUF_B_INDEX_CUR: case BUF_B_CELL_START: case BUF_B_CELL_END: case BUF_B_SORTED: case BUF_BD_BODY_SORTED: break;
        }
        return nullptr;
    }

    static int ev_begin(const Step &s, int stage) { return s.timer->begin(stage, false, s.profMask, s.stream); }
    static int ev_end(const Step &s) { return s.timer->end(s.stream); }

    // ---- the launch rule ------------------------------------------------------------------------------------------------------------------
    // The one place that chooses between the reference-order launch and the list-driven one.  The list kernels use the Muller gradient:
    // they exist for the Muller kernels only (plan.lists is never set for a Monaghan build, Features::listKernels).  So `lists` is a
    // generic callable, called with the kernel set as a std::integral_constant and naming its kernels by it: what it names is
    // instantiated where it is called, here, under `if constexpr`.
    template <typename Ref, typename Lists> static void ref_or_lists(const Step &s, Ref &&ref, Lists &&lists)
    {
        if (!s.plan.lists) ref();
        else if constexpr (KSET == KS_MULLER) lists(std::integral_constant<int, KSET>{});
    }
    // One neighbour launch over the sorted slots.  ref: the reference-order kernel, taking (head..., tail...).  kernels(ks, w): the list
    // kernel of kernel set ks with (w true) or without wall workgroups, taking (head..., hit lists, tail..., wall list, wall workgroups):
    //   WALL_GROUPS   wall workgroups over this step's wall list + interior workgroups without the boundary code, as the scan (grid +
    //                 wall_blocks) when plan.walls; else interior workgroups only
    //   INTERIOR_ONLY the launch walks fluid neighbours only: always the plain kernel
    //   NO_WALL_ARGS  ... and the kernel has no wall parameters at all
    // tail: one of SortedArrays' subsets.
    enum WallMode { WALL_GROUPS, INTERIOR_ONLY, NO_WALL_ARGS };
    template <WallMode WM, typename Ref, typename Kernels, typename... H, typename... T>
    static void gather(const Step &s, Ref ref, Kernels kernels, const std::tuple<H...> &head, const std::tuple<T...> &tail)
    {
        const dim3 g(nblocks(s.sorted.N)), b(BLOCK);
        ref_or_lists(
            s, [&] { std::apply([&](const auto &...a) { hipLaunchKernelGGL(ref, g, b, 0, s.stream, a...); }, std::tuple_cat(head, tail)); },
            [&](auto ks) {
                std::apply(
                    [&](const auto &...a) {
                        if constexpr (WM == WALL_GROUPS) {
                            if (s.plan.walls) {
                                const auto walled = kernels(ks, std::true_type{});
                                const uint32_t wb = wall_blocks(g.x);
                                hipLaunchKernelGGL(walled, dim3(g.x + wb), b, 0, s.stream, a..., s.walls, wb);
                                return;
                            }
                        }
                        const auto plain = kernels(ks, std::false_type{});
                        if constexpr (WM == NO_WALL_ARGS) hipLaunchKernelGGL(plain, g, b, 0, s.stream, a...);
                        else hipLaunchKernelGGL(plain, g, b, 0, s.stream, a..., WallList{}, 0u);
                    },
                    std::tuple_cat(head, std::tie(s.hb), tail));
            });
    }
    // One neighbour pass of PCISPH, PBF, DFSPH or the Akinci normals (nrs_kernels_walk.h): with wall workgroups where the pass has a
    // boundary term, one plain launch where it walks fluid neighbours only.
    template <bool HAS_B, typename Pass> static void launch_pass(const Step &s, const Pass &pass)
    {
        constexpr bool B = HAS_B && Pass::WALLED;
        gather<Pass::WALLED ? WALL_GROUPS : INTERIOR_ONLY>(s, k_walk_ref<Pass, B>, [](auto, auto w) { return k_walk_lists<Pass, B, w>; }, std::tie(pass, s.G), s.sorted.p());
    }
    // The one neighbourhood scan of an IISPH, PCISPH, PBF or DFSPH step, whose hit lists drive the rest of the chain
    // (nrs_kernels_iisph.h).  The scan opens `stage`; the caller ends it.
    template <bool HAS_B> static int density_scan(const Step &s, int stage)
    {
        const SortedArrays<R> &a = s.sorted;
        NRSCHK(ev_begin(s, stage));
        ref_or_lists(
            s, [&] { hipLaunchKernelGGL((k_density_ref<R, KSET, HAS_B>), dim3(nblocks(a.N)), dim3(BLOCK), 0, s.stream, s.P, s.G, a.pos, a.dens, (R *)nullptr, a.N); },
            [&](auto ks) { launch_density_wide<R, ks, HAS_B>(s.stream, s.P, s.G, s.thr, s.hb, a.pos, a.dens, a.N, s.plan.walls ? &s.walls : (const WallList *)nullptr); });
        return NRS_OK;
    }
    // iisph_integrate (sph_cuda.cu:857-867) of velAdv + forcesP, timed as `stage`: the last launch of an IISPH, PCISPH or DFSPH step
    template <typename Last> int integrate_adv(const Step &s, int stage, Last &&last)
    {
        const SortedArrays<R> &a = s.sorted;
        NRSCHK(ev_begin(s, stage));
        return last(s.plan, [&](uint32_t *nh, uint32_t *ni, const uint32_t *prevHash, uint32_t *tileMovers) {
            hipLaunchKernelGGL((k_iisph_integrate<R>), dim3(nblocks(a.N)), dim3(BLOCK), 0, s.stream, s.P, a.pos, a.vel, velAdv.as<T4>(),
                               forcesP.as<T4>(), a.N, nh, ni, prevHash, tileMovers, s.slab ? 1 : 0);
        });
    }

    // ---- IISPH (nrs_kernels_iisph.h; DESIGN.md "IISPH") ------------------------------------------------------------------------------------
    IisphArrays<R> iisph_view(const Step &s) const
    {
        IisphArrays<R> I;
        I.densAdv = densAdv.as<R>(); I.densCorr = densCorr.as<R>(); I.P_l = P_l.as<R>(); I.P_l_next = P_l2.as<R>();
        I.aii = aii.as<R>();
        I.velAdv = velAdv.as<T4>(); I.forcesAdv = forcesAdv.as<T4>(); I.forcesP = forcesP.as<T4>();
        I.diiF = diiF.as<T4>(); I.diiB = diiB.as<T4>(); I.sumDij = sumDij.as<T4>(); I.diiSum = diiSum.as<T4>();
        I.inv = inv.as<uint32_t>();
        I.nonFinite = s.plan.watch ? s.nonFinite : (uint32_t *)nullptr;
        return I;
    }
    // predictAdvection (sph_cuda.cu:513-697)
    template <bool HAS_B> int iisph_predict(const Step &s, int stop)
    {
        const IisphArrays<R> I = iisph_view(s);
        NRSCHK(density_scan<HAS_B>(s, NRS_STAGE_I_DENSITY));
        NRSCHK(ev_end(s));
        if (stop == NRS_STAGE_I_DENSITY) return NRS_OK;
        NRSCHK(ev_begin(s, NRS_STAGE_I_DISPLACEMENT));
        gather<WALL_GROUPS>(s, k_displacement_ref<R, KSET, SURF, HAS_B>, [](auto ks, auto w) { return k_displacement_lists<R, ks, SURF, HAS_B, w>; },
                            std::tie(s.P, s.G, I), s.sorted.pvdp());
        NRSCHK(ev_end(s));
        if (stop == NRS_STAGE_I_DISPLACEMENT) return NRS_OK;
        NRSCHK(ev_begin(s, NRS_STAGE_I_ADVECTION));
        gather<WALL_GROUPS>(s, k_advection_ref<R, KSET, HAS_B>, [](auto ks, auto w) { return k_advection_lists<R, ks, HAS_B, w>; }, std::tie(s.P, s.G, I),
                            s.sorted.pvdp());
        NRSCHK(ev_end(s));
        iisphIter = 0;
        return NRS_OK;
    }
    // one relaxed-Jacobi iteration of pressureSolve (sph_cuda.cu:736-823): sum d_ij p_j, pressure update (double-buffered P_l)
    template <bool HAS_B> int iisph_iteration(const Step &s)
    {
        const IisphArrays<R> I = iisph_view(s);
        gather<NO_WALL_ARGS>(s, k_sumdij_ref<R, KSET>, [](auto ks, auto) { return k_sumdij_lists<R, ks>; }, std::tie(s.P, s.G, I), s.sorted.pd());
        gather<WALL_GROUPS>(s, k_pressure_ref<R, KSET, HAS_B>, [](auto ks, auto w) { return k_pressure_lists<R, ks, HAS_B, w>; }, std::tie(s.P, s.G, I),
                            s.sorted.pdp());
        std::swap(P_l.p, P_l2.p);
        ++iisphIter;
        return NRS_OK;
    }
    // computePressureForce + iisph_integrate (sph_cuda.cu:827-867)
    template <bool HAS_B, typename Last> int iisph_finish(const Step &s, int stop, Last &&last)
    {
        const IisphArrays<R> I = iisph_view(s);
        NRSCHK(ev_begin(s, NRS_STAGE_I_PFORCE));
        gather<WALL_GROUPS>(s, k_pforce_ref<R, KSET, HAS_B>, [](auto ks, auto w) { return k_pforce_lists<R, ks, HAS_B, w>; }, std::tie(s.P, s.G, I),
                            s.sorted.pdp());
        NRSCHK(ev_end(s));
        if (stop == NRS_STAGE_I_PFORCE) return NRS_OK;
        return integrate_adv(s, NRS_STAGE_I_INTEGRATE, last);
    }
    // The list-driven chain is the reference-order chain only while every value a neighbour gathers is finite (IisphArrays::nonFinite;
    // the context clears the word before the chain).  A solve that overflows raises the flag; the step is then repeated from the sorted
    // input with the reference-order kernels, so that even a diverging run produces what the reference's loops produce (plan.watch).
    template <bool HAS_B, typename Last> int iisph_tail(const Step &s, int stop, Last &&last)
    {
        NRSCHK(iisph_tail_once<HAS_B>(s, stop, last));
        if (!s.plan.watch || !iisphDiverged) return NRS_OK;
        Step again = s;
        again.plan = s.repeat;
        ++iisphRestarts;
        hipLaunchKernelGGL((k_gather_scalar<R>), dim3(nblocks(s.sorted.N)), dim3(BLOCK), 0, s.stream, s.presA, s.sortIndex, s.sorted.pres, s.sorted.N);
        return iisph_tail_once<HAS_B>(again, stop, last);
    }
    template <bool HAS_B, typename Last> int iisph_tail_once(const Step &s, int stop, Last &&last)
    {
        const bool watch = s.plan.watch;
        // the flag, read back and waited for; with acc: in the round trip of the density-error sum, whose wait covers it
        auto measure = [&](double *acc, uint32_t *flag) {
            if (flag) HIPCHK(hipMemcpyAsync(flag, s.nonFinite, 4, hipMemcpyDeviceToHost, s.stream));
            if (acc) return red.sum(densCorr.as<R>(), s.sorted.N, acc);
            HIPCHK(hipStreamSynchronize(s.stream));
            return (int)NRS_OK;
        };
        iisphDiverged = false;
        NRSCHK(iisph_predict<HAS_B>(s, stop));
        if (stop && stop <= NRS_STAGE_I_ADVECTION) {
            uint32_t hflag = 0u;
            if (watch) NRSCHK(measure(nullptr, &hflag));
            iisphDiverged = hflag != 0u;
            return NRS_OK;
        }
        // pressureSolve (sph_cuda.cu:702-899); its exit rule: iisph_loop (nrs_host_plan.h)
        NRSCHK(ev_begin(s, NRS_STAGE_I_SOLVE));
        uint32_t l = 0;
        NRSCHK(iisph_loop<R>(s.sorted.N, s.maxIters, watch, [&] { return iisph_iteration<HAS_B>(s); }, measure, &l, &iisphDiverged));
        *s.iters = l;
        NRSCHK(ev_end(s));
        if (iisphDiverged) return NRS_OK; // (the caller repeats the step in reference order)
        if (stop == NRS_STAGE_I_SOLVE) return NRS_OK;
        return iisph_finish<HAS_B>(s, stop, last);
    }

    // ---- PCISPH (nrs_kernels_pcisph.h; DESIGN.md "PCISPH") -----------------------------------------------------------------------------------
    void *pci_xs_current() const { return pciSt.xs ? posPred2.p : posPred.p; }
    PciArrays<R> pci_view(int in, int out) const
    {
        PciArrays<R> A;
        A.velAdv = velAdv.as<T4>(); A.forcesAdv = forcesAdv.as<T4>(); A.forcesP = forcesP.as<T4>();
        A.densPred = densCorr.as<R>(); A.pres = P_l.as<R>(); A.err = pciErr.as<R>();
        A.xsIn = (in ? posPred2 : posPred).as<T4>();
        A.xsOut = (out ? posPred2 : posPred).as<T4>();
        A.delta = pciSt.delta();
        return A;
    }
    // delta from the prototype's sums (k_pci_prototype, the solver's own W_grad on the device; pci_delta) unless it was given; once per
    // parameter or settings change
    int pcisph_prepare(const Params<R> &P, hipStream_t stream)
    {
        if (pciSt.delta_valid()) return NRS_OK;
        const double m = (double)P.particleMass, rd = (double)P.restDensity, given = pciSt.s.deltaGiven;
        double o[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (!(given > 0.0))
            NRSCHK(prototype_sums(P, true, pciSt.s.spacing > 0.0 ? pciSt.s.spacing : prototype_default_spacing(m, rd), "PCISPH", "pressure scale delta", o, stream));
        R d;
        NRSCHK(pci_delta(given, o, (double)P.timestep, m, rd, &d));
        pciSt.set_delta(d);
        return NRS_OK;
    }
    // the advection launch with the Akinci model on (nrs_kernels_akinci.h); SURF_EFF: the context's fsurf term, off while gamma > 0
    template <bool HAS_B, bool SURF_EFF> static void akinci_advect(const Step &s, const PciArrays<R> &A0, const AkinciView<R> &K)
    {
        gather<WALL_GROUPS>(s, k_akinci_advect_ref<R, KSET, SURF_EFF, HAS_B>, [](auto ks, auto w) { return k_akinci_advect_lists<R, ks, SURF_EFF, HAS_B, w>; },
                            std::tie(s.P, s.G, A0, K), s.sorted.pvdp());
    }
    // the density scan and the advection launch of a PCISPH, PBF or DFSPH step (x*0 into posPred); *more = false when the step stops here
    template <bool HAS_B> int pci_prefix(const Step &s, int stop, bool *more)
    {
        *more = false;
        NRSCHK(density_scan<HAS_B>(s, NRS_STAGE_DENSITY));
        if (dfsph()) dfsph_factor<HAS_B>(s);
        NRSCHK(ev_end(s));
        if (stop == NRS_STAGE_DENSITY) return NRS_OK;
        NRSCHK(ev_begin(s, NRS_STAGE_P_ADVECT));
        if (dfsph()) { // the divergence solve on the sorted velocities: the advection reads divergence-free ones
            dfSt.divIters = 0;
            if (dfSt.s.minItersV)
                NRSCHK((dfsph_solve<HAS_B, false>(s, s.sorted.vel, dfKvB.as<R>(), dfErrV.as<R>(), dfSt.s.minItersV, dfSt.s.etaV, &dfSt.divIters)));
            dfSt.divN = dfSt.s.minItersV ? s.sorted.N : 0u;
        }
        pciSt.xs = 0;
        const PciArrays<R> A0 = pci_view(0, 0);
        const bool cohesion = akSt.s.gamma > 0.0;
        if (cohesion || (HAS_B && akSt.s.beta > 0.0)) { // the Akinci model: the normals launch, then the advection launch with its walk
            const AkinciView<R> K{cohesion ? akNormals.as<T4>() : (T4 *)nullptr, (R)akSt.s.gamma, (R)akSt.s.beta};
            if (cohesion) {
                launch_pass<HAS_B>(s, AkinciNormalsPass<R, KSET>{s.P, s.sorted.dens, K.normals});
                akSt.normalsValid = true;
            }
            if (SURF && !cohesion) akinci_advect<HAS_B, SURF>(s, A0, K);
            else akinci_advect<HAS_B, false>(s, A0, K);
        } else {
            gather<WALL_GROUPS>(s, k_pci_advect_ref<R, KSET, SURF, HAS_B>, [](auto ks, auto w) { return k_pci_advect_lists<R, ks, SURF, HAS_B, w>; },
                                std::tie(s.P, s.G, A0), s.sorted.pvdp());
        }
        if (dfsph() && visc.on()) // the implicit viscosity solve on vel_adv (DESIGN.md "Implicit viscosity")
            NRSCHK(visc.solve(red, s.P, velAdv.as<T4>(), s.sorted.dens, s.sorted.N, s.stream, [&](auto start, const ViscArrays<R> &A) {
                launch_pass<HAS_B>(s, ViscMatvecPass<R, KSET, decltype(start)::value>{s.P, A});
            }));
        NRSCHK(ev_end(s));
        *more = stop != NRS_STAGE_P_ADVECT;
        return NRS_OK;
    }
    template <bool HAS_B, typename Last> int pcisph_tail(const Step &s, int stop, Last &&last)
    {
        const uint32_t N = s.sorted.N;
        bool more;
        NRSCHK(pci_prefix<HAS_B>(s, stop, &more));
        if (!more) return NRS_OK;
        // the predictive-corrective loop: stop after the iteration l with l >= min_iters and max e <= eta, or at the cap; the max is
        // not formed (nor read back) before min_iters
        NRSCHK(ev_begin(s, NRS_STAGE_P_SOLVE));
        uint32_t l = 0;
        double err = -1.0;
        NRSCHK(solve_loop(
            false, pciSt.s.minIters, s.maxIters ? s.maxIters : 50u, pciSt.s.eta,
            [&](uint32_t) {
                const PciArrays<R> A = pci_view(pciSt.xs, pciSt.xs ^ 1);
                launch_pass<HAS_B>(s, PciDensityPass<R, KSET>{s.P, A});
                gather<WALL_GROUPS>(s, k_pci_pforce_ref<R, KSET, HAS_B>, [](auto ks, auto w) { return k_pci_pforce_lists<R, ks, HAS_B, w>; }, // (hand-written, nrs_kernels_pcisph.h)
                                    std::tie(s.P, s.G, A), s.sorted.p());
                pciSt.xs ^= 1;
            },
            [&](double *e) { return red.template max_of<false>(pciErr.p, N, e); }, &l, &err));
        *s.iters = l;
        pciSt.lastErr = err;
        HIPCHK(hipMemcpyAsync(s.sorted.pres, P_l.p, sizeof(R) * N, hipMemcpyDeviceToDevice, s.stream)); // (the step's pressures, NRS_ARR_PRES)
        NRSCHK(ev_end(s));
        if (stop == NRS_STAGE_P_SOLVE) return NRS_OK;
        return integrate_adv(s, NRS_STAGE_P_INTEGRATE, last);
    }

    // ---- PBF (nrs_kernels_pbf.h; DESIGN.md "PBF") ---------------------------------------------------------------------------------------------
    PbfArrays<R> pbf_view(int in, int out) const
    {
        PbfArrays<R> A;
        A.densPred = densCorr.as<R>(); A.lambda = P_l.as<R>(); A.err = pciErr.as<R>();
        A.dx = forcesP.as<T4>();
        A.xsIn = (in ? posPred2 : posPred).as<T4>();
        A.xsOut = (out ? posPred2 : posPred).as<T4>();
        A.eps = pbfSt.eps();
        return A;
    }
    // W_q = W((dq h, 0, 0)) on the device (k_pbf_wq), with the current parameters
    int pbf_eval_wq(const Params<R> &P, double dq, R *wq, hipStream_t stream)
    {
        hipLaunchKernelGGL((k_pbf_wq<R, KSET>), dim3(1), dim3(64), 0, stream, P, (R)dq, red.scratch());
        HIPCHK(hipGetLastError());
        double o = 0.0;
        NRSCHK(red.read_scratch(&o, 1));
        if (!(o > 0.0) || !std::isfinite(o)) return fail(NRS_E_INVALID, "PBF tensile correction: W((dq h, 0, 0)) is not positive");
        *wq = (R)o;
        return NRS_OK;
    }
    // The five prototype sums (nrs_host_solver.h "the derived constants") of a particle on the cubic lattice of the given spacing, by
    // k_pci_prototype or k_pbf_prototype: the solver's own gradient on the device.  At least one neighbour, or an error.
    int prototype_sums(const Params<R> &P, bool pci, double spacing, const char *who, const char *what, double *o, hipStream_t stream)
    {
        const double h = (double)P.interactionRadius;
        const R sp = (R)spacing;
        int kmax;
        NRSCHK(prototype_lattice((double)sp, h, who, &kmax));
        if (pci) hipLaunchKernelGGL((k_pci_prototype<R, KSET>), dim3(1), dim3(64), 0, stream, P, sp, kmax, red.scratch());
        else hipLaunchKernelGGL((k_pbf_prototype<R, KSET>), dim3(1), dim3(64), 0, stream, P, sp, kmax, red.scratch());
        HIPCHK(hipGetLastError());
        NRSCHK(red.read_scratch(o, 5));
        return prototype_has_neighbours(o, (double)sp, h, who, what);
    }
    // D of PBF's prototype on the default lattice (eps = relaxation * D, DFSPH's threshold = 1e-6 D)
    int pbf_prototype_d(const Params<R> &P, const char *who, const char *what, double *d, hipStream_t stream)
    {
        double o[5];
        NRSCHK(prototype_sums(P, false, prototype_default_spacing((double)P.particleMass, (double)P.restDensity), who, what, o, stream));
        *d = prototype_d(o);
        return NRS_OK;
    }
    // W_q and eps, each once per change of the parameters or settings it depends on
    int pbf_prepare(const Params<R> &P, hipStream_t stream)
    {
        if (pbfSt.s.tensK > 0.0 && !pbfSt.wq_valid()) {
            R wq;
            NRSCHK(pbf_eval_wq(P, pbfSt.s.tensDq, &wq, stream));
            pbfSt.set_wq(wq);
        }
        if (pbfSt.eps_valid()) return NRS_OK;
        double d;
        NRSCHK(pbf_prototype_d(P, "PBF", "eps", &d, stream));
        R e;
        NRSCHK(pbf_eps(pbfSt.s.relax, d, &e));
        pbfSt.set_eps(e);
        return NRS_OK;
    }
    template <bool HAS_B, typename Last> int pbf_tail(const Step &s, int stop, Last &&last)
    {
        const SortedArrays<R> &a = s.sorted;
        const uint32_t N = a.N;
        bool more;
        NRSCHK(pci_prefix<HAS_B>(s, stop, &more));
        if (!more) return NRS_OK;
        // Jacobi projection: with eta > 0 stop after the iteration l with l >= min_iters and max e <= eta, or at the cap, the max not
        // formed (nor read back) before min_iters; with eta = 0 exactly min_iters iterations and no read-back at all
        NRSCHK(ev_begin(s, NRS_STAGE_P_SOLVE));
        const bool fixed = pbfSt.s.eta == 0.0;
        const uint32_t cap = fixed ? pbfSt.s.minIters : (s.maxIters ? s.maxIters : 50u);
        const bool tens = pbfSt.s.tensK > 0.0;
        const PbfTensile<R> T{(R)pbfSt.s.tensK, pbfSt.wq()};
        uint32_t l = 0;
        double err = -1.0;
        NRSCHK(solve_loop(
            fixed, pbfSt.s.minIters, cap, pbfSt.s.eta,
            [&](uint32_t) {
                const PbfArrays<R> A = pbf_view(pciSt.xs, pciSt.xs ^ 1);
                launch_pass<HAS_B>(s, PbfLambdaPass<R, KSET>{s.P, A});
                if (tens) launch_pass<HAS_B>(s, PbfCorrectPass<R, KSET, true>{s.P, A, T});
                else launch_pass<HAS_B>(s, PbfCorrectPass<R, KSET, false>{s.P, A, {}});
                pciSt.xs ^= 1;
            },
            [&](double *e) { return red.template max_of<false>(pciErr.p, N, e); }, &l, &err));
        *s.iters = l;
        pciSt.lastErr = err;
        pbfSt.errPending = fixed ? N : 0u;
        HIPCHK(hipMemcpyAsync(a.pres, P_l.p, sizeof(R) * N, hipMemcpyDeviceToDevice, s.stream)); // (lambda, NRS_ARR_PRES)
        NRSCHK(ev_end(s));
        if (stop == NRS_STAGE_P_SOLVE) return NRS_OK;
        // v = (x* - x) / dt (+ XSPH), x = x*.  The XSPH launch reads x_j and x*_j of its neighbours, so it leaves the velocities in velB
        // and k_pbf_integrate, which overwrites x, follows it.
        NRSCHK(ev_begin(s, NRS_STAGE_P_INTEGRATE));
        const T4 *xs = (const T4 *)pci_xs_current();
        const bool xsph = pbfSt.s.xsph > 0.0, vort = pbfSt.s.vortEps > 0.0;
        if (xsph) launch_pass<HAS_B>(s, PbfXsphPass<R, KSET>{{}, s.P, xs, a.vel, (R)pbfSt.s.xsph});
        // vorticity confinement: omega from u = (x* - x) / dt, then the confinement on the velocity XSPH left (or u); both read x_j
        if (vort) {
            T4 *om = pbfVort.as<T4>();
            const int given = xsph ? 1 : 0;
            launch_pass<HAS_B>(s, PbfVorticityPass<R, KSET>{{}, s.P, xs, om});
            launch_pass<HAS_B>(s, PbfConfinePass<R, KSET>{{}, s.P, xs, (const T4 *)om, a.vel, given, (R)pbfSt.s.vortEps});
            pbfSt.vortValid = true;
        }
        return last(s.plan, [&](uint32_t *nh, uint32_t *ni, const uint32_t *prevHash, uint32_t *tileMovers) {
            hipLaunchKernelGGL((k_pbf_integrate<R>), dim3(nblocks(N)), dim3(BLOCK), 0, s.stream, s.P, a.pos, a.vel, xs, (xsph || vort) ? 1 : 0, N, nh, ni,
                               prevHash, tileMovers);
        });
    }

    // ---- DFSPH (nrs_kernels_dfsph.h; DESIGN.md "DFSPH") ----------------------------------------------------------------------------------------
    // HASH .. DENSITY as PCISPH (then the factor launch), P_ADVECT = the divergence solve + PCISPH's advection launch, P_SOLVE = the
    // density solve on vel_adv, P_INTEGRATE = integrate_adv (Fp = 0: v = vel_adv, x += dt v)
    DfsphArrays<R> dfsph_view(const Step &s, T4 *u, R *K, R *err) const
    {
        DfsphArrays<R> A;
        A.u = u; A.dens = s.sorted.dens; A.alpha = dfAlpha.as<R>(); A.kappa = P_l.as<R>(); A.K = K; A.err = err;
        A.rhoAdv = densCorr.as<R>(); A.thr = dfSt.threshold();
        return A;
    }
    // thr = 1e-6 D_proto, D_proto = |sum g|^2 + sum |g|^2 of PBF's prototype (k_pbf_prototype); once per parameter change
    int dfsph_prepare(const Params<R> &P, hipStream_t stream)
    {
        if (dfSt.threshold_valid()) return NRS_OK;
        double d;
        NRSCHK(pbf_prototype_d(P, "DFSPH", "D_proto", &d, stream));
        R thr;
        NRSCHK(dfsph_threshold(d, &thr));
        dfSt.set_threshold(thr);
        return NRS_OK;
    }
    template <bool HAS_B> void dfsph_factor(const Step &s)
    {
        launch_pass<HAS_B>(s, DfsphFactorPass<R, KSET>{{s.P, dfsph_view(s, nullptr, nullptr, nullptr)}});
        dfSt.alphaValid = true;
    }
    // one A/B pair on u
    template <bool HAS_B, bool DENS> static void dfsph_pair(const Step &s, const DfsphArrays<R> &A, int phase)
    {
        const DfsphPassBase<R, KSET> base{s.P, A};
        const bool moving = HAS_B && s.movingWalls; // A with the wall velocities (DfsphDivPass's MOVING); B is unchanged
        if constexpr (HAS_B) {
            if (moving) launch_pass<HAS_B>(s, DfsphDivPass<R, KSET, DENS, true>{base, s.wallVel, phase});
        }
        if (!moving) launch_pass<HAS_B>(s, DfsphDivPass<R, KSET, DENS>{base, {}, phase});
        gather<WALL_GROUPS>(s, k_dfsph_vupdate_ref<R, KSET, HAS_B>, [](auto ks, auto w) { return k_dfsph_vupdate_lists<R, ks, HAS_B, w>; }, // B: hand-written (nrs_kernels_dfsph.h)
                            std::tie(s.P, s.G, A), s.sorted.p());
    }
    // one solve (DENS: the density solve) in place on u, K in place on K (the sorted K_prev on entry).  eta > 0: stop after the iteration
    // l with l >= min_iters and avg e <= eta, or at the cap (nrs_set_max_iterations, 0 = 100), the average not formed (nor read back)
    // before min_iters; eta = 0: exactly min_iters iterations and no read-back.  The warm-start pair counts as no iteration.
    template <bool HAS_B, bool DENS> int dfsph_solve(const Step &s, T4 *u, R *K, R *err, uint32_t minIters, double eta, uint32_t *iters)
    {
        const uint32_t N = s.sorted.N;
        const DfsphArrays<R> A = dfsph_view(s, u, K, err);
        const bool fixed = eta == 0.0;
        const uint32_t cap = fixed ? minIters : (s.maxIters ? s.maxIters : 100u);
        if (dfSt.s.warm) dfsph_pair<HAS_B, DENS>(s, A, DFSPH_PHASE_WARM);
        double avg = 0.0;
        return solve_loop(
            fixed, minIters, cap, eta, [&](uint32_t l) { dfsph_pair<HAS_B, DENS>(s, A, (l || dfSt.s.warm) ? DFSPH_PHASE_MORE : DFSPH_PHASE_FIRST); },
            [&](double *e) {
                double acc = 0.0;
                NRSCHK(red.sum(err, N, &acc));
                *e = acc / (double)N;
                return (int)NRS_OK;
            },
            iters, &avg);
    }
    template <bool HAS_B, typename Last> int dfsph_tail(const Step &s, int stop, Last &&last)
    {
        bool more;
        NRSCHK(pci_prefix<HAS_B>(s, stop, &more));
        if (!more) return NRS_OK;
        NRSCHK(ev_begin(s, NRS_STAGE_P_SOLVE));
        uint32_t l = 0;
        NRSCHK((dfsph_solve<HAS_B, true>(s, velAdv.as<T4>(), s.sorted.pres, pciErr.as<R>(), dfSt.s.minIters, dfSt.s.eta, &l)));
        *s.iters = l;
        dfSt.denN = s.sorted.N;
        NRSCHK(ev_end(s));
        if (stop == NRS_STAGE_P_SOLVE) return NRS_OK;
        return integrate_adv(s, NRS_STAGE_P_INTEGRATE, last);
    }
};

} // namespace nrs
