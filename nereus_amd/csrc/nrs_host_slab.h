// nrs_host_slab.h — the host decisions of the slab exchange (nrs_slab_configure / _pack / _unpack): which cell-table window a rank
// keeps, which calls nrs_slab_configure refuses, which form the partition takes, what the stream totals of a pack mean and where the
// pieces of an unpack go.  No HIP: plain integers and bools in, plain integers out.  The exchange's owner (SlabExchange<R>,
// nrs_slab_exchange.h) holds one SlabHost and launches the kernels; the context (nrs_ctx_impl.h) reads it through that owner and applies
// what these functions return to n, nOwned and the state of the particle arrays (array_state()).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

#include "nrs_error.h"
#include "nrs_host_grid.h"
#include "nrs_host_solver.h"

namespace nrs {

// The argument refusals of nrs_slab_configure.  IISPH: every solver iteration consumes two cells of halo validity, the predict stages
// three and the pressure force one: 2 iterations — the reference's minimum — need 8 cells.
static inline int slab_refuse_configure(int solver, bool hasBodies, int lo, int hi, int halo)
{
    if (hasBodies) return fail(NRS_E_INVALID, "contexts with boundary bodies have no slab decomposition");
    if (const char *name = predictive_solver_name(solver)) return fail(NRS_E_INVALID, std::string(name) + " contexts have no slab decomposition");
    if (solver == NRS_SOLVER_IISPH && halo < 8) return fail(NRS_E_INVALID, "IISPH slabs need a halo of at least 8 cells (2 * iterations + 4)");
    if (halo < 2) return fail(NRS_E_INVALID, "halo must be >= 2 cells (one cell for the density of the ring + one)");
    if ((long long)hi - lo < 2ll * halo) return fail(NRS_E_INVALID, "slab narrower than two halos");
    return NRS_OK;
}

// The form a partition takes; the values are what NRS_STAT_SLAB_PARTITION reports.
enum class SlabForm : int {
    COMPACT = 0,       // the owned particles are compacted into the B arrays
    INPLACE = 1,       // they stay where they are; dead slots get the key 0xffffffff (AS_HOLES until the next reorder)
    PRECLASSIFIED = 2  // in place, and the force kernel of the last step already classified every slot for these cuts
};
struct SlabFacts {
    bool classifiedValid, slotOrderValid; // the context's flags of those names
    bool resortBuffers;                   // the coherent re-sort's buffers exist
    bool hashCur, hashNext, hashDistinct; // the sorted keys / the fused kernel's keys per slot are there, and in different buffers
    uint32_t classifiedN, N;
    uint64_t resortMin; // RESORT_MIN_PARTICLES
};
struct SlabChoice {
    SlabForm form;
    bool resort; // the pack counts the owned particles that stay but changed cell (COMPACT: next to a compacted copy of the old keys)
};
static inline SlabChoice choose_form(const SlabFacts &f)
{
    if (f.N == 0) return {SlabForm::COMPACT, false};
    // coherent re-sort of the next step: possible when the arrays are still in the slot order of the last sort and the fused force
    // kernel left the new keys per slot ...
    const bool resort = f.resortBuffers && f.slotOrderValid && f.hashCur && f.hashNext && f.hashDistinct;
    if (resort && f.classifiedValid && f.classifiedN == f.N) return {SlabForm::PRECLASSIFIED, true};
    // ... and then the owned particles need not be moved at all
    return {resort && (uint64_t)f.N >= f.resortMin ? SlabForm::INPLACE : SlabForm::COMPACT, resort};
}

// the stream totals of a pack, in the order of nrs_kernels_slab.h's ST_* (nrs_slab_exchange.h asserts that they agree)
enum { SLT_STAY = 0, SLT_MIG_L = 1, SLT_HALO_L = 2, SLT_MIG_R = 3, SLT_HALO_R = 4, SLT_GHOST = 5, SLT_COUNT = 6, SLT_CHANGED = 6, SLT_TOTALS = 7 };

struct SlabFinish { // what SlabHost::finish hands the context; valid when `stored`
    bool stored = false;
    uint32_t n = 0;      // particles that stay
    SlabForm form = SlabForm::COMPACT;
    uint32_t movers = 0; // of them, those that changed cell
};
struct SlabArrivals { // what SlabHost::unpack hands the context
    bool inplace = false;   // the arrays still have the holes of an in-place partition
    uint32_t start[6] = {0, 0, 0, 0, 0, 0}; // AppendPieces::start: migrants from the left, from the right, our ghosts, halo from the left, from the right
    uint64_t base = 0, arrivals = 0; // first free physical slot, particles appended there
    uint64_t n = 0, nOwned = 0;      // of the next step
};

struct SlabHost {
    // ---- the cell-table window [winBase, winBase + winW) of cell-x columns covering the slab, its halo, two columns of drift and
    // WINDOW_SLACK columns of room for moving cuts; choose_window returns true when it changed.  force: choose afresh (the global
    // grid changed).
    int winBase = 0;
    uint32_t winW = 0; // 0: no window
    static constexpr int WINDOW_SLACK = 8;
    static bool pow2(uint32_t v) { return v && !(v & (v - 1)); }
    bool choose_window(const uint32_t grid[3], int lo, int hi, int halo, bool force)
    {
        const long long GX = (long long)grid[0];
        long long a = std::max<long long>(0, (long long)lo - halo - 2), b = std::min<long long>(GX, (long long)hi + halo + 2);
        if (!(pow2(grid[0]) && pow2(grid[1]) && pow2(grid[2])) || b <= a) {
            const bool changed = winW != 0;
            winW = 0; winBase = 0;
            return changed;
        }
        if (!force && winW && a >= winBase && b <= (long long)winBase + (long long)winW) return false; // still fits
        a = std::max<long long>(0, a - WINDOW_SLACK); b = std::min<long long>(GX, b + WINDOW_SLACK);
        const uint32_t w = next_pow2((uint32_t)(b - a));
        const int baseOld = winBase; const uint32_t wOld = winW;
        if (w >= (uint32_t)GX) { winW = 0; winBase = 0; }
        else { winW = w; winBase = (int)a; }
        return winW != wOld || winBase != baseOld;
    }

    // ---- the last pack: what nrs_slab_pack leaves for finish() (the host half of the pack, run when the totals are needed) ...
    bool pending = false; // its totals have not been looked at yet
    bool packed = false;  // there has been a pack: form is its form
    SlabForm form = SlabForm::COMPACT;
    bool resort = false;  // SlabChoice::resort, until the unpack has used it
    uint32_t N = 0;       // particles it partitioned
    uint64_t mcap = 0;    // particles per message buffer
    // ... and what finish() leaves for the unpack, nrs_slab_last_counts and the statistics
    uint32_t totals[SLT_TOTALS] = {0, 0, 0, 0, 0, 0, 0};
    bool inplace() const { return form != SlabForm::COMPACT; }
    void queue(SlabChoice c, uint32_t N_, uint64_t mcap_)
    {
        pending = true; packed = true;
        form = c.form; resort = c.resort; N = N_; mcap = mcap_;
    }
    // raw: the seven totals of k_slab_scan; scanChanged / scanDead: the cell changers and dead slots the re-sort's scan totalled
    // (read in the pre-classified form only, where the force kernel counted per tile what k_slab_count would have).  An
    // overflowing message is reported after the results have been stored: the counts tell the caller how much room it needs.
    int finish(const uint32_t raw[SLT_TOTALS], uint32_t scanChanged, uint32_t scanDead, SlabFinish &out)
    {
        out = SlabFinish();
        pending = false;
        uint32_t tot[SLT_TOTALS] = {0, 0, 0, 0, 0, 0, 0};
        if (N) {
            std::memcpy(tot, raw, sizeof(tot));
            if (form == SlabForm::PRECLASSIFIED) {
                tot[SLT_CHANGED] = scanChanged;
                tot[SLT_STAY] = N - scanDead;
            }
        }
        if ((uint64_t)tot[SLT_STAY] + tot[SLT_MIG_L] + tot[SLT_MIG_R] > N || tot[SLT_CHANGED] > tot[SLT_STAY])
            return fail(NRS_E_HIP, "inconsistent slab stream totals");
        std::memcpy(totals, tot, sizeof(tot));
        out.stored = true;
        out.n = tot[SLT_STAY]; out.form = form; out.movers = tot[SLT_CHANGED];
        if ((uint64_t)tot[SLT_MIG_L] + tot[SLT_HALO_L] > mcap || (uint64_t)tot[SLT_MIG_R] + tot[SLT_HALO_R] > mcap || tot[SLT_GHOST] > mcap)
            return fail(NRS_E_CAPACITY, "slab message capacity exceeded");
        return NRS_OK;
    }
    // hL / hR: the 16-byte headers of the received messages (migrants, halo copies, 0, 0), null for a missing one.  n, physN, holes:
    // the context's live count, the physical extent of its arrays and whether they still have holes; cap: its capacity.
    int unpack(const uint32_t *hL, const uint32_t *hR, uint64_t n, uint32_t physN, bool holes, uint64_t msgCap, uint64_t cap, SlabArrivals &a) const
    {
        const uint32_t none[4] = {0, 0, 0, 0};
        if (!hL) hL = none;
        if (!hR) hR = none;
        if ((uint64_t)hL[0] + hL[1] > msgCap || (uint64_t)hR[0] + hR[1] > msgCap) return fail(NRS_E_INVALID, "corrupt slab message header");
        a = SlabArrivals();
        a.inplace = inplace() && holes;
        const uint32_t len[5] = {hL[0], hR[0], totals[SLT_GHOST], hL[1], hR[1]};
        for (int k = 0; k < 5; ++k) {
            a.start[k + 1] = a.start[k] + len[k];
            a.arrivals += len[k];
        }
        a.base = a.inplace ? (uint64_t)physN : n;
        if (a.base + a.arrivals > cap) return fail(NRS_E_CAPACITY, "owned + halo particles exceed the context capacity");
        a.nOwned = n + hL[0] + hR[0];
        a.n = n + a.arrivals; // live particles of the next step
        return NRS_OK;
    }
};

} // namespace nrs
