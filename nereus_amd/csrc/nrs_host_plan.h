// nrs_host_plan.h — which kernels a step launches, and the exit rules of the solver loops.  No HIP: the flags, the solver, the build's
// precision and kernel set and a few grid facts in, a plan out.  The context (nrs_ctx_impl.h) fills PlanFacts, keeps the plan of the
// step in progress and launches by it, as do the solver chains it hands the plan to (nrs_solvers.h), which run the loops.
#pragma once
#include <cstdint>

#include "nrs_error.h"
#include "nrs_host_state.h"

namespace nrs {

// The flag- and type-derived half of the choice is fixed at init() and decides which optional buffers exist (init(),
// rebuild_boundary_tables()); plan_step() adds the grid facts of the step.  The launch sites read the plan, nothing else.
struct PlanFacts {
    uint32_t flags; // nrs_config.flags
    int solver;     // nrs_config.solver
    bool muller;    // KSET == KS_MULLER
    bool fp32;      // R is float
    uint64_t cap, n;
    bool qOk;           // the geometry allows the compact scan candidates (scan_quant, nrs_host_scan.h)
    bool pow2Grid;      // every extent of the grid is a power of two
    bool nearBitsValid; // the wall buffers exist and nearBits describes the current grid
    bool walls;         // nb != 0
    bool slabOn;
    uint32_t numCells;  // of the kernels' grid (P.numCells)
};
struct Features {
    bool listKernels; // the solver has list-driven kernels for this kernel set (IISPH, PCISPH: Muller only, the Monaghan support is 2h)
    bool lists;       // hitBuf, hitCounts, qpos (+ gatherPos for SESPH)
    bool fast;        // fastQ
    bool resort;      // the coherent re-sort buffers
};
static inline Features plan_features(const PlanFacts &a)
{
    const uint32_t f = a.flags;
    const bool sesph = a.solver == NRS_SOLVER_SESPH;
    Features ft;
    ft.listKernels = sesph || a.muller;
    ft.lists = ft.listKernels && !(f & (NRS_FLAG_REFERENCE_ORDER | NRS_FLAG_NO_SHARED_LISTS));
    ft.fast = ft.lists && (f & NRS_FLAG_FAST_ARITH) && sesph && a.fp32 && a.muller;
    ft.resort = !(f & (NRS_FLAG_REFERENCE_ORDER | NRS_FLAG_NO_FUSION | NRS_FLAG_FULL_SORT)) && a.cap >= RESORT_MIN_PARTICLES;
    return ft;
}
struct StepPlan {
    bool ref = true;        // reference-order kernels; none of the fields below except quant
    bool quant = false;     // the reorder writes qpos and the grid view hands it to the scans
    bool lists = false;     // the density scan builds hit lists and the gathers after it consume them
    bool wallTiles = false; // the reorder counts the wall slots per tile ...
    bool walls = false;     // ... and the wall list is built: the gathers run wall workgroups + interior workgroups
    bool staged = false;    // SESPH: the LDS-staged density launch
    bool fast = false;      // SESPH: fast arithmetic in the force walk
    bool keys = false;      // the step's last launch writes the next step's sort keys (SESPH: the fused force launch)
    bool resort = false;    // ... and counts the movers: the split of the coherent re-sort is queued behind it
    bool classify = false;  // ... and classifies for the next slab partition
    bool watch = false;     // IISPH: the list-driven chain flags non-finite gathers (IisphArrays::nonFinite, iisph_tail)
};
static inline StepPlan plan_step(const PlanFacts &a, int stop, bool ref)
{
    const Features ft = plan_features(a);
    const bool sesph = a.solver == NRS_SOLVER_SESPH, iisph = a.solver == NRS_SOLVER_IISPH;
    StepPlan s;
    // the tiled kernels assume the power-of-two grids the reference's hash assumes (sph_kernel_impl.cuh:120)
    s.ref = ref || (a.flags & NRS_FLAG_REFERENCE_ORDER) || !a.pow2Grid;
    // hit lists are built (and the kernels that consume them used) only when the scan that builds them can run
    s.quant = ft.lists && a.qOk;
    if (s.ref) return s;
    // SESPH: density -> forces, shared only when the step goes on past the density; IISPH, PCISPH: one scan feeds the chain
    // (nrs_kernels_iisph.h, nrs_kernels_pcisph.h)
    s.lists = s.quant && (!sesph || stop != NRS_STAGE_DENSITY);
    // LDS-staged density scan (nrs_kernels_staged.h): fp32 SESPH on power-of-two grids.  Measured at 10 M particles it is
    // SLOWER than the global-memory scan in the exact arithmetic (0.84 vs 0.71 ms: the kernel is bound by vector-instruction
    // issue, not by the latency the staging removes), and since the quantised scan (0.52 ms) also slower than the
    // exact path in its own fast arithmetic (0.70-0.88 ms): it runs only when NRS_FLAG_STAGED_SCAN asks for it.
    s.staged = (a.flags & NRS_FLAG_STAGED_SCAN) && a.fp32 && a.muller && sesph && s.quant && a.numCells <= (1u << 30);
    // fast arithmetic (reciprocals, rsq, fused multiply-adds) in the FORCE walk: fp32 Muller SESPH with shared lists; the density
    // kernel (exact) leaves the (p/rho^2, 1/rho) pairs it needs; everything else keeps IEEE arithmetic
    s.fast = ft.fast && s.lists;
    // wall workgroups (nrs_kernels_tiled.h): the scan and the gathers over its lists (SESPH forces; IISPH displacement, advection,
    // pressure, pressure force).  The reorder counts the tiles even when the step stops after the density; the staged launch
    // has no wall workgroups.
    s.wallTiles = !(a.flags & NRS_FLAG_NO_WALL_WORKGROUPS) && a.nearBitsValid && a.walls && s.quant && !s.staged;
    s.walls = s.wallTiles && s.lists;
    // a full step also leaves the next step's sort keys (and the split of the coherent re-sort) — IISPH not in slab runs, whose
    // arrays are re-partitioned first
    s.keys = stop == 0 && !(a.flags & NRS_FLAG_NO_FUSION) && !(iisph && a.slabOn);
    const bool resort = s.keys && ft.resort && a.n >= RESORT_MIN_PARTICLES;
    s.resort = resort && !a.slabOn;
    // slab runs: the next partition's classification rides in the same launch (k_slab_count and most of k_slab_scatter then have
    // nothing left to do)
    s.classify = resort && a.slabOn;
    // (not in slab runs, whose loop the host drives; PCISPH has no reference-order repeat)
    s.watch = iisph && s.lists && !a.slabOn;
    return s;
}

// The exit rule of the three solver loops: iterate(l) queues iteration l (from 0); after min_iters iterations measure(&e) reads the
// error measure back, and the loop stops on e <= eta or at the cap.  fixed: exactly `cap` iterations and nothing read back.
template <typename Iterate, typename Measure>
int solve_loop(bool fixed, uint32_t minIters, uint32_t cap, double eta, Iterate &&iterate, Measure &&measure, uint32_t *iters, double *err)
{
    uint32_t l = 0;
    for (;;) {
        iterate(l);
        ++l;
        const bool last = l >= cap;
        if (fixed) {
            if (last) break;
        } else if (l >= minIters || last) {
            NRSCHK(measure(err));
            if (last || *err <= eta) break;
        }
    }
    *iters = l;
    return NRS_OK;
}

// IISPH's exit rule, the reference's (pressureSolve, sph_cuda.cu:702-899): while ((rho_avg - 1000) > 1 || l < 2), evaluated in the
// solver's precision R, or until maxIters (0: no cap) iterations.  iterate() queues one iteration.  The loop condition reads rho_avg
// only once l >= 2 (sph_cuda.cu:736: `|| l < 2`): the average of the first iteration is never looked at, so nothing is reduced or read
// back after it.  measure(&acc, flag) forms the sum of the N density errors (rho_avg = (R)acc / N, in R) and waits for it; flag, unless
// null, gets the word the list-driven chain raises on a non-finite gather (watch; StepPlan::watch), which rides in the same round
// trip and ends the loop when set.  measure(nullptr, flag) reads the word alone: once, behind the loop, when the last iteration did no
// reduction.  *flagged: the word was set; the caller repeats the step in reference order.
template <typename R, typename Iterate, typename Measure>
int iisph_loop(uint32_t N, uint32_t maxIters, bool watch, Iterate &&iterate, Measure &&measure, uint32_t *iters, bool *flagged)
{
    uint32_t l = 0, hflag = 0u;
    R rho_avg = 0.f;
    const R rd = 1000.f;
    const R max_rho_err = 1.f;
    bool flagRead = false;
    while (((rho_avg - rd) > max_rho_err) || (l < 2)) {
        NRSCHK(iterate());
        l++;
        flagRead = false;
        if (maxIters && l >= maxIters) break;
        if (l >= 2) {
            double acc = 0.0;
            NRSCHK(measure(&acc, watch ? &hflag : (uint32_t *)nullptr));
            flagRead = true;
            if (watch && hflag) break;
            rho_avg = (R)acc;
            rho_avg /= N;
        }
    }
    if (watch && !flagRead) NRSCHK(measure((double *)nullptr, &hflag));
    *iters = l;
    *flagged = watch && hflag != 0u;
    return NRS_OK;
}

} // namespace nrs
