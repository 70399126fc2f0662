// host_parts_main.cpp — stand-alone driver of the library's HIP-free host components (nrs_host_bodies.h, nrs_host_settings.h,
// nrs_host_slab.h, nrs_host_state.h, nrs_host_plan.h, nrs_host_solver.h, nrs_host_grid.h) for tests/test_host_parts_cpu.py, tests/test_host_state_cpu.py
// and tests/test_host_solver_cpu.py: one command per line on stdin, one answer per line on stdout (the commands that enumerate a cross
// product themselves answer with one word or line per case, in the order stated at the command).  Doubles travel as C99 hex floats (or
// nan / inf), so nothing is rounded on the way.  Built by the test with the host compiler, plain and under the sanitizers.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "nrs_host_bodies.h"
#include "nrs_host_grid.h"
#include "nrs_host_plan.h"
#include "nrs_host_settings.h"
#include "nrs_host_slab.h"
#include "nrs_host_solver.h"
#include "nrs_host_state.h"

namespace nrs {
thread_local std::string g_err;
}
using namespace nrs;

static void put(const double *v, int n)
{
    for (int i = 0; i < n; ++i) printf(" %a", v[i]);
}
static void answer(int rc)
{
    if (rc == NRS_OK) printf("rc 0\n");
    else printf("rc %d %s\n", rc, g_err.c_str());
}

// one transition of the tracker: op numbers in the order nrs_host_state.h declares them, a / b its arguments (0 where it has none)
static void apply(ArrayTracker &t, int op, uint32_t a, uint32_t b)
{
    switch (op) {
    case 0: t.drop_prepared_keys(); break;
    case 1: t.to_fresh(); break;
    case 2: t.keys_ready(); break;
    case 3: t.split_queued(); break;
    case 4: t.split_queued_known(a); break;
    case 5: t.to_holes(a, b); break;
    case 6: t.holes_consumed(); break;
    case 7: t.holes_compacted(); break;
    case 8: t.grid_changed(); break;
    case 9: t.classification_dropped(); break;
    case 10: t.classified(a); break;
    case 11: t.cuts_changed(); break;
    case 12: t.pack_hashed(a != 0); break;
    case 13: t.arrivals_appended(a != 0, b); break;
    case 14: t.step_ended(a != 0); break;
    default: fprintf(stderr, "host_parts_main: unknown transition %d\n", op); exit(2);
    }
}
static unsigned field_bits(const ArrayFields &f)
{
    return (f.hashReady ? 1u : 0u) | (f.rsPending ? 2u : 0u) | (f.rsCountKnown ? 4u : 0u) | (f.slotOrderValid ? 8u : 0u) | (f.classifiedValid ? 16u : 0u) |
           (f.holesPending ? 32u : 0u) | (f.packedHashValid ? 64u : 0u);
}

// nrs_host_solver.h: the buffers by the names the context gives them, the units as v / s / u (x n), c (u32 x numCells), vb / ub (x nb)
static const char *buf_name(BufName b)
{
    static const char *const names[] = {
        "none", "posA", "posB", "velA", "velB", "presA", "presB", "dens", "forces", "hashCur", "indexCur", "cellStart", "cellEnd", "bHashCur",
        "bIndexCur", "bCellStart", "bCellEnd", "bSorted", "bdBodySorted", "inv", "densAdv", "P_l2", "aii", "diiF", "diiB", "sumDij", "diiSum",
        "velAdv", "forcesAdv", "forcesP", "densCorr", "P_l", "posPred", "posPred2", "pciErr", "dfAlpha", "dfKvA", "dfKvB", "dfErrV", "pbfVort",
        "akNormals"};
    static_assert(sizeof(names) / sizeof(names[0]) == BUF_COUNT, "one name per BufName");
    return names[b];
}
static const char *unit_name(ArrayUnit u)
{
    static const char *const names[] = {"v", "s", "u", "c", "vb", "ub"};
    return names[u];
}
static const char *stat_name(StatKind k)
{
    static const char *const names[] = {"movers", "slabForm", "pbfError", "pbfEps", "dfDivIters", "dfMax", "dfAvg", "pciError", "pciDelta",
                                        "hitOverflow", "hitMean", "hitMax", "unstaged"};
    static_assert(sizeof(names) / sizeof(names[0]) == STAT_HIT_UNSTAGED + 1, "one name per StatKind");
    return names[k];
}
// delta / eps / thr in the context's precision: the neighbour test of the prototype's sums, then the formula
template <typename R> static void derived(const std::string &cmd, const std::vector<double> &a)
{
    int rc;
    R out = (R)0;
    if (cmd == "delta") { // delta prec given o0 .. o4 sp h dt m rho0
        rc = a[1] > 0.0 ? (int)NRS_OK : prototype_has_neighbours(&a[2], a[7], a[8], "PCISPH", "pressure scale delta");
        if (rc == NRS_OK) rc = pci_delta<R>(a[1], &a[2], a[9], a[10], a[11], &out);
    } else if (cmd == "eps") { // eps prec relax o0 .. o4 sp h
        rc = prototype_has_neighbours(&a[2], a[7], a[8], "PBF", "eps");
        if (rc == NRS_OK) rc = pbf_eps<R>(a[1], prototype_d(&a[2]), &out);
    } else { // thr prec o0 .. o4 sp h
        rc = prototype_has_neighbours(&a[1], a[6], a[7], "DFSPH", "D_proto");
        if (rc == NRS_OK) rc = dfsph_threshold<R>(prototype_d(&a[1]), &out);
    }
    if (rc == NRS_OK) printf("rc 0 %a\n", (double)out);
    else answer(rc);
}

// grid prec h n x y z ...: the bounding box of the n points and the grid it asks for, in the context's precision (the numbers given are
// values of that precision).  Answers rc, then origin, extents and cell count: of a grid holding 7 everywhere if the call refused
template <typename R> static void grid(const std::vector<double> &a)
{
    const uint64_t n = (uint64_t)a[2];
    std::vector<R> p4(4 * n, (R)1);
    for (uint64_t i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) p4[4 * i + c] = (R)a[3 + 3 * i + c];
    R mn[3], mx[3];
    aabb_of_points(p4.data(), n, mn, mx);
    AabbGrid<R> g = {{(R)7, (R)7, (R)7}, {7u, 7u, 7u}, 7u};
    answer(grid_from_aabb(mn, mx, (R)a[1], g));
    printf("grid %a %a %a %u %u %u %u\n", (double)g.origin[0], (double)g.origin[1], (double)g.origin[2], g.size[0], g.size[1], g.size[2], g.numCells);
}

// iloop prec N maxIters watch flagFrom acc0 acc1 ...: IISPH's exit rule in the context's precision.  The k-th reduction answers acc_k
// (the last one again once they run out); the watch word reads 1 from iteration flagFrom on (0: never).  Answers rc, then iterate
// calls, iters, whether the loop reports the word set, and every measure call: r = the sum, f = the word, then the iterations done
template <typename R> static void iloop(const std::vector<double> &a)
{
    const uint32_t N = (uint32_t)a[1], maxIters = (uint32_t)a[2], flagFrom = (uint32_t)a[4];
    uint32_t iterates = 0, iters = 12345u;
    size_t k = 5;
    bool flagged = false;
    std::string calls;
    const int rc = iisph_loop<R>(
        N, maxIters, a[3] != 0.0, [&] { ++iterates; return (int)NRS_OK; },
        [&](double *acc, uint32_t *flag) {
            calls += std::string(" ") + (acc ? "r" : "") + (flag ? "f" : "") + std::to_string(iterates);
            if (flag) *flag = (flagFrom && iterates >= flagFrom) ? 1u : 0u;
            if (acc) *acc = a[std::min(k++, a.size() - 1)];
            return (int)NRS_OK;
        },
        &iters, &flagged);
    answer(rc);
    printf("iloop %u %u %d%s\n", iterates, iters, flagged ? 1 : 0, calls.c_str());
}

int main()
{
    BodyPoses bodies;
    PciSettings pci;
    PbfSettings pbf;
    DfsphSettings df;
    AkinciSettings ak;
    SlabHost sx;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        if (!(in >> cmd)) continue;
        std::vector<double> a;
        while (in >> tok) a.push_back(strtod(tok.c_str(), nullptr));
        auto need = [&](size_t n) {
            if (a.size() == n) return;
            fprintf(stderr, "host_parts_main: '%s' takes %zu numbers, got %zu\n", cmd.c_str(), n, a.size());
            exit(2);
        };
        if (cmd == "init") { // init nbodies cx cy cz ... : one particle per body at the given point
            const uint32_t nb = a.empty() ? 0u : (uint32_t)a[0];
            if (nb > (uint32_t)NRS_MAX_BODIES) { fprintf(stderr, "host_parts_main: too many bodies\n"); return 2; }
            need(1 + 3 * (size_t)nb);
            double sum[NRS_MAX_BODIES][3] = {{0.0}};
            uint64_t cnt[NRS_MAX_BODIES] = {0};
            for (uint32_t k = 0; k < nb; ++k) {
                for (int c = 0; c < 3; ++c) sum[k][c] = a[1 + 3 * k + c];
                cnt[k] = 1;
            }
            bodies.init(nb, sum, cnt);
            answer(NRS_OK);
        } else if (cmd == "vel") {
            need(7);
            answer(bodies.set_velocity((uint32_t)a[0], &a[1], &a[4]));
        } else if (cmd == "pose") {
            need(8);
            answer(bodies.set_pose((uint32_t)a[0], &a[1], &a[4]));
        } else if (cmd == "get") {
            need(1);
            double x[3], q[4];
            const int rc = bodies.get_pose((uint32_t)a[0], x, q);
            if (rc != NRS_OK) { answer(rc); continue; }
            printf("pose");
            put(x, 3); put(q, 4);
            printf("\n");
        } else if (cmd == "rot") {
            need(1);
            double r[9];
            bodies.rotation((uint32_t)a[0], r);
            printf("rot");
            put(r, 9);
            printf("\n");
        } else if (cmd == "adv") { // adv dt steps
            need(2);
            for (int s = 0; s < (int)a[1]; ++s) bodies.advance(a[0]);
            answer(NRS_OK);
        } else if (cmd == "rebuilt") { // what the context does once the boundary tables stand at the poses
            bodies.dirty = false;
            answer(NRS_OK);
        } else if (cmd == "clear") {
            bodies.clear();
            answer(NRS_OK);
        } else if (cmd == "state") {
            printf("state %u %d %d %d %d\n", bodies.n, bodies.moving() ? 1 : 0, bodies.displaced() ? 1 : 0, bodies.dirty ? 1 : 0,
                   bodies.n > 1 && BodyPoses::has_velocity(bodies.b[1]) ? 1 : 0);
        } else if (cmd == "pci") {
            need(4);
            answer(pci.set(a[0], (uint32_t)a[1], a[2], a[3]));
            printf("pci %a %u %a %a\n", pci.eta, pci.minIters, pci.spacing, pci.deltaGiven);
        } else if (cmd == "pbf") {
            need(4);
            answer(pbf.set(a[0], (uint32_t)a[1], a[2], a[3]));
            printf("pbf %a %u %a %a\n", pbf.eta, pbf.minIters, pbf.relax, pbf.xsph);
        } else if (cmd == "tens") {
            need(2);
            answer(pbf.set_tensile(a[0], a[1]));
            printf("tens %a %a\n", pbf.tensK, pbf.tensDq);
        } else if (cmd == "vort") {
            need(1);
            answer(pbf.set_vorticity(a[0]));
            printf("vort %a\n", pbf.vortEps);
        } else if (cmd == "df") {
            need(5);
            answer(df.set(a[0], (uint32_t)a[1], a[2], (uint32_t)a[3], (int)a[4]));
            printf("df %a %u %a %u %d\n", df.eta, df.minIters, df.etaV, df.minItersV, df.warm ? 1 : 0);
        } else if (cmd == "ak") {
            need(2);
            answer(ak.set(a[0], a[1]));
            printf("ak %a %a\n", ak.gamma, ak.beta);
        } else if (cmd == "win") { // win gx gy gz lo hi halo force
            need(7);
            const uint32_t grid[3] = {(uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2]};
            const bool changed = sx.choose_window(grid, (int)a[3], (int)a[4], (int)a[5], a[6] != 0.0);
            printf("win %d %d %u\n", changed ? 1 : 0, sx.winBase, sx.winW);
        } else if (cmd == "form") { // form classifiedValid slotOrderValid resortBuffers hashCur hashNext hashDistinct classifiedN N resortMin
            need(9);
            const SlabChoice c = choose_form(SlabFacts{a[0] != 0.0, a[1] != 0.0, a[2] != 0.0, a[3] != 0.0, a[4] != 0.0, a[5] != 0.0, (uint32_t)a[6],
                                                       (uint32_t)a[7], (uint64_t)a[8]});
            printf("form %d %d\n", (int)c.form, c.resort ? 1 : 0);
        } else if (cmd == "cfg") { // cfg solver has_bodies lo hi halo
            need(5);
            answer(slab_refuse_configure((int)a[0], a[1] != 0.0, (int)a[2], (int)a[3], (int)a[4]));
        } else if (cmd == "queue") { // queue form resort N message_capacity: what nrs_slab_pack leaves behind
            need(4);
            sx.queue(SlabChoice{(SlabForm)(int)a[0], a[1] != 0.0}, (uint32_t)a[2], (uint64_t)a[3]);
            answer(NRS_OK);
        } else if (cmd == "fin") { // fin t0 .. t6 scan_changed scan_dead
            need(9);
            uint32_t raw[SLT_TOTALS];
            for (int k = 0; k < SLT_TOTALS; ++k) raw[k] = (uint32_t)a[k];
            SlabFinish f;
            answer(sx.finish(raw, (uint32_t)a[7], (uint32_t)a[8], f));
            printf("fin %d %u %d %u %d", f.stored ? 1 : 0, f.n, (int)f.form, f.movers, sx.pending ? 1 : 0);
            for (int k = 0; k < SLT_TOTALS; ++k) printf(" %u", sx.totals[k]);
            printf("\n");
        } else if (cmd == "unp") { // unp has_left migrants halo has_right migrants halo n physN holes message_capacity capacity
            need(11);
            const uint32_t hL[4] = {(uint32_t)a[1], (uint32_t)a[2], 0, 0}, hR[4] = {(uint32_t)a[4], (uint32_t)a[5], 0, 0};
            SlabArrivals r;
            const int rc = sx.unpack(a[0] != 0.0 ? hL : nullptr, a[3] != 0.0 ? hR : nullptr, (uint64_t)a[6], (uint32_t)a[7], a[8] != 0.0, (uint64_t)a[9],
                                     (uint64_t)a[10], r);
            answer(rc);
            if (rc == NRS_OK)
                printf("unp %d %u %u %u %u %u %u %llu %llu %llu %llu\n", r.inplace ? 1 : 0, r.start[0], r.start[1], r.start[2], r.start[3], r.start[4],
                       r.start[5], (unsigned long long)r.base, (unsigned long long)r.arrivals, (unsigned long long)r.n, (unsigned long long)r.nOwned);
        } else if (cmd == "astates") {
            // astates n cap nOwned physN known: the state for every mask of 12 bits, bit k of the mask being, from 0: hashReady rsPending
            // rsCountKnown slotOrderValid classifiedValid holesPending | slabOn inplace hashNext indexNext hashCur rsMovers
            need(5);
            std::string out(4096, '?');
            for (unsigned m = 0; m < 4096u; ++m) {
                auto bit = [&](int k) { return ((m >> k) & 1u) != 0; };
                ArrayFields f;
                f.hashReady = bit(0); f.rsPending = bit(1); f.rsCountKnown = bit(2); f.slotOrderValid = bit(3); f.classifiedValid = bit(4);
                f.holesPending = bit(5); f.physN = (uint32_t)a[3]; f.rsKnownCount = (uint32_t)a[4];
                const ArrayFacts facts = {(uint64_t)a[0], (uint64_t)a[1], (uint64_t)a[2], bit(6), bit(7), bit(8), bit(9), bit(10), bit(11)};
                out[m] = (char)('0' + (int)array_state(f, facts));
            }
            printf("astates %s\n", out.c_str());
        } else if (cmd == "seqs") { // seqs depth n cap nOwned (op a b)...: every sequence of 0 .. depth of the given transitions from the
            // initial fields, shorter ones first, each length in the order of counting with the first transition as the most
            // significant digit; one line per sequence: field bits, known count, classifiedN, physN, state under the given facts
            // (slab run, in place, every pointer there)
            if (a.size() < 4 || (a.size() - 4) % 3) { fprintf(stderr, "host_parts_main: seqs depth n cap nOwned (op a b)...\n"); return 2; }
            const size_t nops = (a.size() - 4) / 3;
            const ArrayFacts facts = {(uint64_t)a[1], (uint64_t)a[2], (uint64_t)a[3], true, true, true, true, true, true};
            for (int len = 0; len <= (int)a[0]; ++len) {
                size_t total = 1;
                for (int k = 0; k < len; ++k) total *= nops;
                for (size_t id = 0; id < total; ++id) {
                    ArrayTracker t;
                    size_t div = total;
                    for (int k = 0; k < len; ++k) {
                        div /= nops;
                        const size_t o = (id / div) % nops;
                        apply(t, (int)a[4 + 3 * o], (uint32_t)a[5 + 3 * o], (uint32_t)a[6 + 3 * o]);
                    }
                    const ArrayFields &f = t.fields();
                    printf("%u %u %u %u %d\n", field_bits(f), f.rsKnownCount, f.classifiedN, f.physN, (int)array_state(f, facts));
                }
            }
            printf("seqs done\n");
        } else if (cmd == "plans") { // plans flag*7 stop*3 cap*3 n*3 cells*2: features and plan as four hex digits per case, the loops
            // nested in this order (outermost first): flag mask (bit k = the k-th flag given), solver 0..4, muller, fp32, the mask of
            // qOk pow2Grid nearBitsValid walls slabOn ref (bit 0..5), stop, cap, n, cells.  Bits of the word, from 0: listKernels lists
            // fast resort | ref quant lists wallTiles walls staged fast keys resort classify watch
            need(18);
            std::string out;
            out.reserve(128u * 5 * 4 * 64 * 3 * 27 * 2 * 4);
            static const char hexd[] = "0123456789abcdef";
            for (unsigned fm = 0; fm < 128u; ++fm) {
                uint32_t flags = 0;
                for (int k = 0; k < 7; ++k) if ((fm >> k) & 1u) flags |= (uint32_t)a[k];
                for (int solver = 0; solver < 5; ++solver)
                    for (int mu = 0; mu < 2; ++mu)
                        for (int f32 = 0; f32 < 2; ++f32)
                            for (unsigned bm = 0; bm < 64u; ++bm)
                                for (int is = 0; is < 3; ++is)
                                    for (int ic = 0; ic < 3; ++ic)
                                        for (int in_ = 0; in_ < 3; ++in_)
                                            for (int ie = 0; ie < 2; ++ie) {
                                                const PlanFacts pf = {flags, solver, mu != 0, f32 != 0, (uint64_t)a[10 + ic], (uint64_t)a[13 + in_],
                                                                      (bm & 1u) != 0, (bm & 2u) != 0, (bm & 4u) != 0, (bm & 8u) != 0, (bm & 16u) != 0,
                                                                      (uint32_t)a[16 + ie]};
                                                const Features ft = plan_features(pf);
                                                const StepPlan s = plan_step(pf, (int)a[7 + is], (bm & 32u) != 0);
                                                const bool b[15] = {ft.listKernels, ft.lists, ft.fast, ft.resort, s.ref, s.quant, s.lists, s.wallTiles,
                                                                    s.walls, s.staged, s.fast, s.keys, s.resort, s.classify, s.watch};
                                                unsigned w = 0;
                                                for (int k = 0; k < 15; ++k) w |= b[k] ? 1u << k : 0u;
                                                for (int k = 3; k >= 0; --k) out.push_back(hexd[(w >> (4 * k)) & 15u]);
                                            }
            }
            printf("plans %s\n", out.c_str());
        } else if (cmd == "sortp") { // sortp holesPending hashReady rsPending rsCountKnown known stop n
            need(7);
            ArrayFields f;
            f.holesPending = a[0] != 0.0; f.hashReady = a[1] != 0.0; f.rsPending = a[2] != 0.0; f.rsCountKnown = a[3] != 0.0;
            f.rsKnownCount = (uint32_t)a[4];
            ResortStats rs;
            const SortPrefix c = choose_sort_prefix(f, (int)a[5], (uint64_t)a[6], rs);
            printf("sortp %d %d %d %d %u %llu %llu %a\n", c.compactFirst ? 1 : 0, c.useKeys ? 1 : 0, c.resort ? 1 : 0, c.countKnown ? 1 : 0, c.knownCount,
                   (unsigned long long)rs.steps, (unsigned long long)rs.fallbacks, rs.lastMovers);
        } else if (cmd == "sortc") { // sortc M N
            need(2);
            ResortStats rs;
            SortKind kind;
            answer(choose_sort((uint64_t)a[0], (uint64_t)a[1], rs, kind));
            printf("sortc %d %llu %llu %a\n", (int)kind, (unsigned long long)rs.steps, (unsigned long long)rs.fallbacks, rs.lastMovers);
        } else if (cmd == "grid") {
            if (a.size() < 6 || a[2] < 1.0 || a.size() != 3 + 3 * (size_t)a[2]) { fprintf(stderr, "host_parts_main: grid prec h n (x y z) * n\n"); return 2; }
            if (a[0] == 64.0) grid<double>(a);
            else grid<float>(a);
        } else if (cmd == "keybits") { // keybits numCells
            need(1);
            printf("keybits %u\n", sort_key_bits((uint32_t)a[0]));
        } else if (cmd == "sparse") { // sparse numCells n
            need(2);
            printf("sparse %d\n", sparse_cell_table((uint64_t)a[0], (uint64_t)a[1]) ? 1 : 0);
        } else if (cmd == "loop") {
            // loop fixed minIters cap eta cross failAt: the error measure is 0.25 from iteration `cross` on (0: never) and 1 + l before;
            // measure fails after iteration failAt (0: never).  Answers rc, then iterate calls, iters (12345: not written), the last
            // error, whether iterate got 0, 1, 2, ... and the iterations after which measure was called
            need(6);
            uint32_t iterates = 0, iters = 12345u;
            double err = -1.0;
            std::vector<uint32_t> measured;
            uint32_t next = 0;
            bool ordered = true;
            const int rc = solve_loop(
                a[0] != 0.0, (uint32_t)a[1], (uint32_t)a[2], a[3],
                [&](uint32_t l) { ordered = ordered && l == next++; ++iterates; },
                [&](double *e) {
                    measured.push_back(iterates);
                    if (a[5] != 0.0 && iterates == (uint32_t)a[5]) return fail(NRS_E_HIP, "measure failed");
                    *e = (a[4] != 0.0 && iterates >= (uint32_t)a[4]) ? 0.25 : 1.0 + (double)iterates;
                    return (int)NRS_OK;
                },
                &iters, &err);
            answer(rc);
            printf("loop %u %u %a %d", iterates, iters, err, ordered ? 1 : 0);
            for (uint32_t l : measured) printf(" %u", l);
            printf("\n");
        } else if (cmd == "iloop") {
            if (a.size() < 6) { fprintf(stderr, "host_parts_main: 'iloop' takes at least 6 numbers\n"); exit(2); }
            if (a[0] == 64.0) iloop<double>(a);
            else iloop<float>(a);
        } else if (cmd == "stage") { // stage solver stop
            need(2);
            answer(stage_allowed((int)a[0], (int)a[1]));
        } else if (cmd == "stale") { // stale old*7 new*7, each: timestep particleMass restDensity interactionRadius kpoly kpoly_grad kpress_grad
            need(14);
            const StaleConstants st = stale_after_params(ParamsKey{a[0], a[1], a[2], a[3], a[4], a[5], a[6]}, ParamsKey{a[7], a[8], a[9], a[10], a[11], a[12], a[13]});
            printf("stale %d %d %d %d\n", st.delta ? 1 : 0, st.eps ? 1 : 0, st.threshold ? 1 : 0, st.wq ? 1 : 0);
        } else if (cmd == "delta" || cmd == "eps" || cmd == "thr") {
            need(cmd == "delta" ? 12 : cmd == "eps" ? 9 : 8);
            if (a[0] == 64.0) derived<double>(cmd, a);
            else derived<float>(cmd, a);
        } else if (cmd == "spacing") { // spacing prec sp h who: the spacing is rounded to the precision first, as the context does
            need(4);
            static const char *const who[] = {"PCISPH", "PBF", "DFSPH"};
            const double sp = a[0] == 64.0 ? a[1] : (double)(float)a[1];
            int kmax = 0;
            const int rc = prototype_lattice(sp, a[2], who[(int)a[3]], &kmax);
            if (rc == NRS_OK) printf("rc 0 %d\n", kmax);
            else answer(rc);
        } else if (cmd == "buffers") { // buffers solver: name:unit:zeroed in the order of allocation
            need(1);
            printf("buffers");
            for (const SolverBuffer &b : solver_buffers((int)a[0])) printf(" %s:%s:%d", buf_name(b.buf), unit_name(b.unit), b.zero ? 1 : 0);
            printf("\n");
        } else if (cmd == "array") {
            // array solver: one line "rc buffer unit | message" per case, the loops nested in this order (outermost first): id -1 .. 40,
            // midStep, walls, bodies, the mask of vortValid normalsValid alphaValid kvValid (bit 0..3), pciXs
            need(1);
            for (int which = -1; which <= 40; ++which)
                for (int mid = 0; mid < 2; ++mid)
                    for (int walls = 0; walls < 2; ++walls)
                        for (int bd = 0; bd < 2; ++bd)
                            for (unsigned m = 0; m < 16u; ++m)
                                for (int xs = 0; xs < 2; ++xs) {
                                    ArrayRoute r = {BUF_NONE, UNIT_VEC4_N};
                                    const int rc = route_array(which, ArrayRouteFacts{(int)a[0], mid != 0, walls != 0, bd != 0, (m & 1u) != 0, (m & 2u) != 0,
                                                                                      (m & 4u) != 0, (m & 8u) != 0, xs}, r);
                                    if (rc != NRS_OK) printf("%d - - | %s\n", rc, g_err.c_str());
                                    else printf("0 %s %s |\n", buf_name(r.buf), r.buf == BUF_NONE ? "0" : unit_name(r.unit));
                                }
            printf("array done\n");
        } else if (cmd == "stat") {
            // stat solver: one line "rc kind divergence count formMaxFirst | message" per case, the loops nested in this order (outermost first): id
            // -1 .. 13, packed, pbfErrPending, solved, dfDenN in {0, 7}, dfDivN in {0, 7}, the mask of hitCounts particles midStep (bit 0..2)
            need(1);
            for (int which = -1; which <= 13; ++which)
                for (int packed = 0; packed < 2; ++packed)
                    for (int pend = 0; pend < 2; ++pend)
                        for (int solved = 0; solved < 2; ++solved)
                            for (uint32_t den = 0; den <= 7u; den += 7u)
                                for (uint32_t dv = 0; dv <= 7u; dv += 7u)
                                    for (unsigned m = 0; m < 8u; ++m) {
                                        StatRoute r;
                                        const int rc = route_stat(which, StatFacts{(int)a[0], packed != 0, pend != 0, solved != 0, den, dv, (m & 1u) != 0,
                                                                                  (m & 2u) != 0, (m & 4u) != 0}, r);
                                        if (rc != NRS_OK) printf("%d - 0 0 0 | %s\n", rc, g_err.c_str());
                                        else printf("0 %s %d %u %d |\n", stat_name(r.kind), r.divergence ? 1 : 0, r.count, r.formMaxFirst ? 1 : 0);
                                    }
            printf("stat done\n");
        } else {
            fprintf(stderr, "host_parts_main: unknown command '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
