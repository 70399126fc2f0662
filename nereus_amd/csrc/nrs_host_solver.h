// nrs_host_solver.h — what differs by solver on the host: which stages a partial step may stop at, which derived constant a parameter
// change makes stale, the constants themselves (PCISPH's delta, PBF's eps, DFSPH's threshold) from the prototype sums, which of the
// shared buffers a solver allocates, and which buffer an array id or which computation a statistic id means on a context — or with
// which text it is refused.  No HIP: solver ids, bools and doubles in, a code and a plain struct out.  The solvers' owner
// (PressureSolvers, nrs_solvers.h) holds one state struct per solver (below), launches the prototype kernels and the reductions and
// maps its buffer names to pointers; the context (nrs_ctx_impl.h) routes arrays and statistics.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "nrs_error.h"
#include "nrs_host_settings.h"

namespace nrs {

// ---- partial-step stages ------------------------------------------------------------------------------------------------------------
// PCISPH, PBF and DFSPH share the stage range of a step (nrs_step_partial) and have no slab decomposition; null for the others
static inline const char *predictive_solver_name(int solver)
{
    return solver == NRS_SOLVER_PCISPH ? "PCISPH" : solver == NRS_SOLVER_PBF ? "PBF" : solver == NRS_SOLVER_DFSPH ? "DFSPH" : nullptr;
}
// stop = 0: a full step
static inline int stage_allowed(int solver, int stop)
{
    const char *const predictive = predictive_solver_name(solver);
    if (predictive && stop && !(stop <= NRS_STAGE_DENSITY || (stop >= NRS_STAGE_P_ADVECT && stop <= NRS_STAGE_P_INTEGRATE)))
        return fail(NRS_E_INVALID, std::string("stage not part of a ") + predictive + " step (HASH .. DENSITY, P_ADVECT .. P_INTEGRATE)");
    return NRS_OK;
}

// ---- which derived constant a parameter change makes stale ----------------------------------------------------------------------------
// The parameters the constants depend on, as doubles (SReal -> double is exact: != means what it meant on the SReal, NaN included;
// the host classes set the parameters every step, so an unchanged set must keep the constants).
struct ParamsKey {
    double timestep, particleMass, restDensity, interactionRadius, kpoly, kpoly_grad, kpress_grad;
};
struct StaleConstants {
    bool delta, eps, threshold, wq; // PCISPH's delta, PBF's eps, DFSPH's threshold, W_q of PBF's tensile correction
};
static inline StaleConstants stale_after_params(const ParamsKey &o, const ParamsKey &q)
{
    const bool mass = q.particleMass != o.particleMass, rho0 = q.restDensity != o.restDensity, h = q.interactionRadius != o.interactionRadius;
    StaleConstants s;
    s.delta = q.timestep != o.timestep || mass || rho0 || h || q.kpoly_grad != o.kpoly_grad;
    s.eps = s.threshold = mass || rho0 || h || q.kpress_grad != o.kpress_grad;
    s.wq = h || q.kpoly != o.kpoly;
    return s;
}

// ---- the derived constants ----------------------------------------------------------------------------------------------------------
// The prototype: a particle on the cubic lattice of spacing sp (default cbrt(m / rho0); the caller rounds it to SReal first, as the
// kernel gets it).  Its five sums over the lattice neighbours within h (k_pci_prototype: g = W_grad; k_pbf_prototype: g = (m / rho0)
// grad W_spiky): o[0..2] = sum g, o[3] = sum g . g, o[4] = neighbours.  `who` and `what` name the caller and its result in the errors.
static inline double prototype_default_spacing(double m, double rho0) { return std::cbrt(m / rho0); }
// the lattice the kernel walks is [-kmax, kmax]^3
static inline int prototype_lattice(double sp, double h, const char *who, int *kmax)
{
    if (!(sp > 0.0) || !std::isfinite(sp) || !(h > 0.0) || h / sp > 64.0) {
        char buf[200];
        snprintf(buf, sizeof(buf), "%s: the prototype spacing (default cbrt(m / rho0)) must be positive and at least h / 64", who);
        return fail(NRS_E_INVALID, buf);
    }
    *kmax = (int)std::ceil(h / sp) + 1;
    return NRS_OK;
}
static inline int prototype_has_neighbours(const double *o, double sp, double h, const char *who, const char *what)
{
    if (o[4] == 0.0) {
        char buf[200];
        snprintf(buf, sizeof(buf), "%s: the prototype particle (lattice spacing %g, h %g) has no neighbour within h: no %s", who, sp, h, what);
        return fail(NRS_E_INVALID, buf);
    }
    return NRS_OK;
}
static inline double prototype_d(const double *o) { return o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3]; } // D = |sum g|^2 + sum |g|^2
// PCISPH: delta = -1 / (beta (-sum g . sum g - sum g . g)), beta = 2 (dt m / rho0)^2; a given delta (> 0) is taken as it is (o unread)
template <typename R> int pci_delta(double deltaGiven, const double *o, double dt, double m, double rho0, R *delta)
{
    if (deltaGiven > 0.0) { *delta = (R)deltaGiven; return NRS_OK; }
    const double q = dt * m / rho0, beta = 2.0 * q * q;
    const double d = -1.0 / (beta * (-(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]) - o[3]));
    if (!std::isfinite(d)) return fail(NRS_E_INVALID, "PCISPH: the prototype gives no finite pressure scale delta");
    *delta = (R)d;
    return NRS_OK;
}
// PBF: eps = relaxation * D
template <typename R> int pbf_eps(double relax, double d, R *eps)
{
    const double e = relax * d;
    if (!(e > 0.0) || !std::isfinite(e)) return fail(NRS_E_INVALID, "PBF: the prototype gives no finite positive eps");
    *eps = (R)e;
    return NRS_OK;
}
// DFSPH: thr = 1e-6 D
template <typename R> int dfsph_threshold(double d, R *thr)
{
    if (!(d > 0.0) || !std::isfinite(d)) return fail(NRS_E_INVALID, "DFSPH: the prototype gives no finite positive D_proto");
    *thr = (R)(1e-6 * d);
    return NRS_OK;
}

// ---- one state struct per solver: settings, derived constants in SReal, whether they belong to the current parameters and settings,
// and what the last step left.  Whether a constant is valid changes through the named methods alone (as ArrayTracker's fields do). -------
template <typename R> struct PciState {
    PciSettings s;
    int xs = 0;            // which of posPred / posPred2 holds the newest predicted positions (PBF's too)
    double lastErr = -1.0; // max e_i after the last iteration of the last solve, PBF's too (< 0: no solve yet)
    R delta() const { return d; }
    bool delta_valid() const { return dValid; } // delta belongs to the current parameters and settings
    void set_delta(R v) { d = v; dValid = true; }
    void settings_changed() { dValid = false; }
    void params_changed(const StaleConstants &st) { if (st.delta) dValid = false; }

private:
    R d = (R)0;
    bool dValid = false;
};
template <typename R> struct PbfState {
    PbfSettings s;
    uint32_t errPending = 0; // fixed-count solve: max e over this many particles is formed on request (get_stat), not in the step
    bool vortValid = false;  // pbfVort holds the omega of a step
    R eps() const { return e; }
    R wq() const { return w; }
    bool eps_valid() const { return eValid; } // eps belongs to the current parameters and settings
    bool wq_valid() const { return wValid; }  // W_q belongs to the current parameters and dq
    void set_eps(R v) { e = v; eValid = true; }
    void set_wq(R v) { w = v; wValid = true; }
    void settings_changed() { eValid = false; }
    void params_changed(const StaleConstants &st)
    {
        if (st.eps) eValid = false;
        if (st.wq) wValid = false;
    }

private:
    R e = (R)0, w = (R)0;
    bool eValid = false, wValid = false;
};
template <typename R> struct DfsphState {
    DfsphSettings s;
    bool alphaValid = false, kvValid = false; // NRS_ARR_DFSPH_ALPHA / _KAPPA_V hold a step's values
    uint32_t denN = 0, divN = 0;              // particles whose e of the last density / divergence iteration pciErr / dfErrV hold (0: none)
    uint32_t divIters = 0;                    // divergence iterations of the last step
    R threshold() const { return t; }
    bool threshold_valid() const { return tValid; } // the threshold belongs to the current parameters
    void set_threshold(R v) { t = v; tValid = true; }
    void params_changed(const StaleConstants &st) { if (st.threshold) tValid = false; }

private:
    R t = (R)0;
    bool tValid = false;
};
struct AkinciState { // gamma = beta_a = 0 is off
    AkinciSettings s;
    bool normalsValid = false; // akNormals holds the records (n_i, rho_i) of a step
};
// (vortValid, alphaValid, kvValid and normalsValid are set by the step that writes the array and never cleared: not by an upload, not
// by a grid change)

// ---- buffers --------------------------------------------------------------------------------------------------------------------------
// The context's buffers by name: what route_array() answers with and solver_buffers() lists.
enum BufName {
    BUF_NONE, // a null pointer
    BUF_POS_A, BUF_POS_B, BUF_VEL_A, BUF_VEL_B, BUF_PRES_A, BUF_PRES_B, BUF_DENS, BUF_FORCES, BUF_HASH_CUR, BUF_INDEX_CUR, BUF_CELL_START, BUF_CELL_END,
    // the boundary's: owned by BoundaryTables (nrs_boundary_tables.h), which maps these six names to pointers itself (buffer())
    BUF_B_HASH_CUR, BUF_B_INDEX_CUR, BUF_B_CELL_START, BUF_B_CELL_END, BUF_B_SORTED, BUF_BD_BODY_SORTED,
    // IISPH only
    BUF_INV, BUF_DENS_ADV, BUF_P_L2, BUF_AII, BUF_DII_F, BUF_DII_B, BUF_SUM_DIJ, BUF_DII_SUM,
    // Shared, and what they hold.  IISPH: its own names.  PCISPH: velAdv, forcesAdv, forcesP, densCorr = rho*, P_l = p, posPred /
    // posPred2 = the two predicted-position buffers, pciErr = the e_i the exit test takes the max of.  PBF: the same, P_l = lambda,
    // forcesP = the last correction dx.  DFSPH: velAdv, forcesAdv, forcesP = 0, densCorr = rho_adv, P_l = kappa, posPred = the
    // advection launch's x* (unused), pciErr = e of the density solve; K lives in presA / presB as IISPH's warm-start pressure does.
    BUF_VEL_ADV, BUF_FORCES_ADV, BUF_FORCES_P, BUF_DENS_CORR, BUF_P_L, BUF_POS_PRED, BUF_POS_PRED2, BUF_PCI_ERR,
    // DFSPH only: alpha, Kv (A: slot order of posA, B: sorted), e of the divergence solve
    BUF_DF_ALPHA, BUF_DF_KV_A, BUF_DF_KV_B, BUF_DF_ERR_V,
    // allocated when the setting is first switched on: PBF's (omega, |omega|), Akinci's (n_i, rho_i)
    BUF_PBF_VORT, BUF_AK_NORMALS,
    BUF_COUNT
};
enum ArrayUnit { UNIT_VEC4_N, UNIT_SCALAR_N, UNIT_U32_N, UNIT_U32_CELLS, UNIT_VEC4_NB, UNIT_U32_NB };

// what a solver allocates at nrs_create (sized by the capacity; UNIT_*_N), in this order, and zero-fills on the stream, in this order
struct SolverBuffer {
    BufName buf;
    ArrayUnit unit;
    bool zero;
};
struct SolverBufferList {
    const SolverBuffer *b;
    int n;
    const SolverBuffer *begin() const { return b; }
    const SolverBuffer *end() const { return b + n; }
};
static inline SolverBufferList solver_buffers(int solver)
{
    static const SolverBuffer iisph[] = {
        {BUF_INV, UNIT_U32_N, false}, {BUF_DENS_ADV, UNIT_SCALAR_N, true}, {BUF_DENS_CORR, UNIT_SCALAR_N, true}, {BUF_P_L, UNIT_SCALAR_N, true},
        {BUF_P_L2, UNIT_SCALAR_N, true}, {BUF_AII, UNIT_SCALAR_N, true}, {BUF_VEL_ADV, UNIT_VEC4_N, true}, {BUF_FORCES_ADV, UNIT_VEC4_N, true},
        {BUF_FORCES_P, UNIT_VEC4_N, true}, {BUF_DII_F, UNIT_VEC4_N, true}, {BUF_DII_B, UNIT_VEC4_N, true}, {BUF_SUM_DIJ, UNIT_VEC4_N, true},
        {BUF_DII_SUM, UNIT_VEC4_N, false}};
    // PCISPH, PBF: no dii / a_ii / sum d_ij p_j, no inverse slot table (the loop skips j == i by sorted slot)
    static const SolverBuffer predictive[] = {
        {BUF_VEL_ADV, UNIT_VEC4_N, true}, {BUF_FORCES_ADV, UNIT_VEC4_N, true}, {BUF_FORCES_P, UNIT_VEC4_N, true}, {BUF_DENS_CORR, UNIT_SCALAR_N, true},
        {BUF_P_L, UNIT_SCALAR_N, true}, {BUF_POS_PRED, UNIT_VEC4_N, true}, {BUF_POS_PRED2, UNIT_VEC4_N, true}, {BUF_PCI_ERR, UNIT_SCALAR_N, true}};
    // DFSPH: PCISPH's advection buffers with one predicted-position buffer, and its own
    static const SolverBuffer dfsph[] = {
        {BUF_VEL_ADV, UNIT_VEC4_N, true}, {BUF_FORCES_ADV, UNIT_VEC4_N, true}, {BUF_FORCES_P, UNIT_VEC4_N, true}, {BUF_DENS_CORR, UNIT_SCALAR_N, true},
        {BUF_P_L, UNIT_SCALAR_N, true}, {BUF_POS_PRED, UNIT_VEC4_N, true}, {BUF_PCI_ERR, UNIT_SCALAR_N, true}, {BUF_DF_ALPHA, UNIT_SCALAR_N, true},
        {BUF_DF_KV_A, UNIT_SCALAR_N, true}, {BUF_DF_KV_B, UNIT_SCALAR_N, true}, {BUF_DF_ERR_V, UNIT_SCALAR_N, true}};
    switch (solver) {
    case NRS_SOLVER_IISPH: return {iisph, (int)(sizeof(iisph) / sizeof(iisph[0]))};
    case NRS_SOLVER_PCISPH:
    case NRS_SOLVER_PBF: return {predictive, (int)(sizeof(predictive) / sizeof(predictive[0]))};
    case NRS_SOLVER_DFSPH: return {dfsph, (int)(sizeof(dfsph) / sizeof(dfsph[0]))};
    default: return {nullptr, 0};
    }
}

// ---- nrs_device_ptr / nrs_get_array: which buffer an array id means -----------------------------------------------------------------
// presA / presB swap at the end of a step (end_of_step), so after a completed step NRS_ARR_PRES is presA: IISPH's warm-start pressure,
// PCISPH's final pressures, PBF's lambda, DFSPH's K
static inline bool pressure_swaps(int solver)
{
    return solver == NRS_SOLVER_IISPH || solver == NRS_SOLVER_PCISPH || solver == NRS_SOLVER_PBF || solver == NRS_SOLVER_DFSPH;
}
struct ArrayRouteFacts {
    int solver;
    bool midStep;                                         // a partial step left the sorted arrays in the B buffers
    bool walls, bodies;                                   // nb != 0; a body assignment
    bool vortValid, normalsValid, alphaValid, kvValid;    // the array holds a step's values
    int pciXs;                                            // the newest predicted positions: posPred (0) or posPred2
};
struct ArrayRoute {
    BufName buf;
    ArrayUnit unit;
};
static inline int route_array(int which, const ArrayRouteFacts &f, ArrayRoute &r)
{
    const bool sesph = f.solver == NRS_SOLVER_SESPH, pcisph = f.solver == NRS_SOLVER_PCISPH, pbf = f.solver == NRS_SOLVER_PBF,
               dfsph = f.solver == NRS_SOLVER_DFSPH;
    const bool sortedIsCurrent = !f.midStep; // after a completed step the sorted arrays ARE the current arrays (buffers were swapped)
    const ArrayUnit v = UNIT_VEC4_N, s = UNIT_SCALAR_N, u = UNIT_U32_N, c = UNIT_U32_CELLS;
    switch (which) {
    case NRS_ARR_POS: r = {BUF_POS_A, v}; break;
    case NRS_ARR_VEL: r = {BUF_VEL_A, v}; break;
    case NRS_ARR_PRESSURE: r = {BUF_PRES_A, s}; break;
    case NRS_ARR_HASH: r = {BUF_HASH_CUR, u}; break;
    case NRS_ARR_INDEX: r = {BUF_INDEX_CUR, u}; break;
    case NRS_ARR_CELL_START: r = {BUF_CELL_START, c}; break;
    case NRS_ARR_CELL_END: r = {BUF_CELL_END, c}; break;
    case NRS_ARR_SORTED_POS: r = {sortedIsCurrent ? BUF_POS_A : BUF_POS_B, v}; break;
    case NRS_ARR_SORTED_VEL: r = {sortedIsCurrent ? BUF_VEL_A : BUF_VEL_B, v}; break;
    case NRS_ARR_DENS: r = {BUF_DENS, s}; break;
    case NRS_ARR_PRES: r = {(pressure_swaps(f.solver) && sortedIsCurrent) ? BUF_PRES_A : BUF_PRES_B, s}; break;
    case NRS_ARR_FORCES: r = {BUF_FORCES, v}; break;
    case NRS_ARR_B_HASH: r = {BUF_B_HASH_CUR, UNIT_U32_NB}; break;
    case NRS_ARR_B_INDEX: r = {BUF_B_INDEX_CUR, UNIT_U32_NB}; break;
    case NRS_ARR_B_CELL_START: r = {f.walls ? BUF_B_CELL_START : BUF_NONE, c}; break;
    case NRS_ARR_B_CELL_END: r = {f.walls ? BUF_B_CELL_END : BUF_NONE, c}; break;
    case NRS_ARR_B_SORTED: r = {BUF_B_SORTED, UNIT_VEC4_NB}; break;
    case NRS_ARR_DENS_ADV: r = {BUF_DENS_ADV, s}; break;
    case NRS_ARR_DENS_CORR: r = {BUF_DENS_CORR, s}; break;
    case NRS_ARR_P_L: r = {BUF_P_L, s}; break;
    case NRS_ARR_AII: r = {BUF_AII, s}; break;
    case NRS_ARR_VEL_ADV: r = {BUF_VEL_ADV, v}; break;
    case NRS_ARR_FORCES_ADV: r = {BUF_FORCES_ADV, v}; break;
    case NRS_ARR_FORCES_P: r = {BUF_FORCES_P, v}; break;
    case NRS_ARR_DII_FLUID: r = {BUF_DII_F, v}; break;
    case NRS_ARR_DII_BOUNDARY: r = {BUF_DII_B, v}; break;
    case NRS_ARR_SUM_DIJ: r = {BUF_SUM_DIJ, v}; break;
    case NRS_ARR_POS_PRED: r = {f.pciXs ? BUF_POS_PRED2 : BUF_POS_PRED, v}; break;
    case NRS_ARR_VORTICITY:
        if (!pbf) return fail(NRS_E_STATE, "PBF array requested from another context");
        if (!f.vortValid) return fail(NRS_E_STATE, "no PBF step with vorticity confinement yet");
        r = {BUF_PBF_VORT, v}; break;
    case NRS_ARR_NORMALS:
        if (!pcisph && !pbf && !dfsph) return fail(NRS_E_STATE, "Akinci array requested from a SESPH or IISPH context");
        if (!f.normalsValid) return fail(NRS_E_STATE, "no step with Akinci surface tension (gamma > 0) yet");
        r = {BUF_AK_NORMALS, v}; break;
    case NRS_ARR_B_BODY: // (not a solver array: none of the per-solver refusals below apply)
        if (!f.bodies) return fail(NRS_E_STATE, "no boundary body assignment (nrs_set_boundary_bodies)");
        r = {BUF_BD_BODY_SORTED, UNIT_U32_NB};
        return NRS_OK;
    case NRS_ARR_DFSPH_ALPHA:
    case NRS_ARR_DFSPH_KAPPA_V:
        if (!dfsph) return fail(NRS_E_STATE, "DFSPH array requested from another context");
        if (which == NRS_ARR_DFSPH_ALPHA) {
            if (!f.alphaValid) return fail(NRS_E_STATE, "no DFSPH factor launch yet");
            r = {BUF_DF_ALPHA, s};
        } else {
            if (!f.kvValid) return fail(NRS_E_STATE, "no DFSPH step yet");
            r = {sortedIsCurrent ? BUF_DF_KV_A : BUF_DF_KV_B, s};
        }
        break;
    default: return fail(NRS_E_INVALID, "unknown array id");
    }
    // the solver arrays (ids from NRS_ARR_DENS_ADV on) a context of another solver refuses; the order decides the text
    if (which == NRS_ARR_POS_PRED && !pcisph && !pbf) return fail(NRS_E_STATE, "PCISPH / PBF array requested from another context");
    const bool shared = which == NRS_ARR_VEL_ADV || which == NRS_ARR_FORCES_ADV || which == NRS_ARR_FORCES_P || which == NRS_ARR_DENS_CORR ||
                        which == NRS_ARR_P_L || which == NRS_ARR_NORMALS;
    const bool pciArray = shared || which == NRS_ARR_POS_PRED || which == NRS_ARR_VORTICITY;
    if (pcisph && which >= NRS_ARR_DENS_ADV && !pciArray) return fail(NRS_E_STATE, "IISPH array requested from a PCISPH context");
    if (pbf && which >= NRS_ARR_DENS_ADV && !pciArray) return fail(NRS_E_STATE, "IISPH array requested from a PBF context");
    const bool dfArray = shared || which == NRS_ARR_DFSPH_ALPHA || which == NRS_ARR_DFSPH_KAPPA_V;
    if (dfsph && which >= NRS_ARR_DENS_ADV && !dfArray) return fail(NRS_E_STATE, "IISPH / PCISPH / PBF array requested from a DFSPH context");
    if (which >= NRS_ARR_DENS_ADV && sesph) return fail(NRS_E_STATE, "IISPH array requested from a SESPH context");
    return NRS_OK;
}

// ---- nrs_get_stat: what a statistic id means ------------------------------------------------------------------------------------------
struct StatFacts {
    int solver;
    bool packed;            // an nrs_slab_pack happened
    bool pbfErrPending;     // PBF, fixed-count solve: the max e of the last solve is still to be formed
    bool solved;            // !(lastErr < 0): a PCISPH / PBF solve left its max e
    uint32_t dfDenN, dfDivN; // DfsphState::denN, divN
    bool hitCounts, particles, midStep; // the shared hit lists exist; n != 0; a partial step is pending
};
enum StatKind {
    STAT_MOVER_COUNT, STAT_SLAB_FORM,
    STAT_PBF_ERROR, STAT_PBF_EPS, STAT_DFSPH_DIV_ITERS,
    STAT_DFSPH_MAX, STAT_DFSPH_AVG, // of `count` values of the density solve's e (pciErr) or, divergence: of the divergence solve's (dfErrV)
    STAT_PCI_ERROR, STAT_PCI_DELTA, STAT_HIT_OVERFLOW, STAT_HIT_MEAN, STAT_HIT_MAX, STAT_HIT_UNSTAGED
};
struct StatRoute {
    StatKind kind;
    bool divergence;
    uint32_t count;
    bool formMaxFirst; // PBF: first form the pending max e (PbfState::errPending particles of pciErr) into lastErr, then ask again
};
static inline int route_stat(int which, const StatFacts &f, StatRoute &r)
{
    const bool pcisph = f.solver == NRS_SOLVER_PCISPH, pbf = f.solver == NRS_SOLVER_PBF, dfsph = f.solver == NRS_SOLVER_DFSPH;
    r = {STAT_MOVER_COUNT, false, 0u, false};
    if (which == NRS_STAT_MOVERS) return NRS_OK;
    if (which == NRS_STAT_SLAB_PARTITION) {
        if (!f.packed) return fail(NRS_E_STATE, "no nrs_slab_pack yet");
        r.kind = STAT_SLAB_FORM;
        return NRS_OK;
    }
    if (pbf && (which == NRS_STAT_DENSITY_ERROR || which == NRS_STAT_PBF_EPSILON)) {
        r.kind = which == NRS_STAT_DENSITY_ERROR ? STAT_PBF_ERROR : STAT_PBF_EPS;
        r.formMaxFirst = f.pbfErrPending; // (fixed-count mode: pciErr still holds the e_i of the last iteration)
        if (!r.formMaxFirst && !f.solved) return fail(NRS_E_STATE, "no PBF solve yet");
        return NRS_OK;
    }
    if (which == NRS_STAT_DFSPH_DENSITY_AVG || which == NRS_STAT_DFSPH_DIVERGENCE_AVG || which == NRS_STAT_DFSPH_DIVERGENCE_ITERATIONS ||
        (dfsph && which == NRS_STAT_DENSITY_ERROR)) {
        if (!dfsph) return fail(NRS_E_STATE, "DFSPH statistic requested from another context");
        if (which == NRS_STAT_DFSPH_DIVERGENCE_ITERATIONS) { r.kind = STAT_DFSPH_DIV_ITERS; return NRS_OK; }
        // formed on request from the e_i the last iteration of the solve left (deterministic: the exit test's own reductions)
        r.divergence = which == NRS_STAT_DFSPH_DIVERGENCE_AVG;
        r.count = r.divergence ? f.dfDivN : f.dfDenN;
        if (!r.count) return fail(NRS_E_STATE, r.divergence ? "no DFSPH divergence solve yet (or it is off)" : "no DFSPH density solve yet");
        r.kind = which == NRS_STAT_DENSITY_ERROR ? STAT_DFSPH_MAX : STAT_DFSPH_AVG;
        return NRS_OK;
    }
    if (which == NRS_STAT_DENSITY_ERROR || which == NRS_STAT_PCISPH_DELTA) {
        if (!pcisph) return fail(NRS_E_STATE, "PCISPH statistic requested from another context");
        if (!f.solved) return fail(NRS_E_STATE, "no PCISPH solve yet");
        r.kind = which == NRS_STAT_DENSITY_ERROR ? STAT_PCI_ERROR : STAT_PCI_DELTA;
        return NRS_OK;
    }
    if (which == NRS_STAT_PBF_EPSILON) return fail(NRS_E_STATE, "PBF statistic requested from another context");
    if (which != NRS_STAT_HIT_OVERFLOW && which != NRS_STAT_HIT_MEAN && which != NRS_STAT_HIT_MAX && which != NRS_STAT_UNSTAGED)
        return fail(NRS_E_INVALID, "unknown statistic");
    if (!f.hitCounts || !f.particles || f.midStep) return fail(NRS_E_STATE, "no shared hit lists (reference-order kernels, or no step yet)");
    r.kind = which == NRS_STAT_HIT_OVERFLOW ? STAT_HIT_OVERFLOW : which == NRS_STAT_HIT_MEAN ? STAT_HIT_MEAN : which == NRS_STAT_HIT_MAX ? STAT_HIT_MAX : STAT_HIT_UNSTAGED;
    return NRS_OK;
}

} // namespace nrs
