// host_inflow_main.cpp — stand-alone driver of the sources' and sinks' HIP-free parts (nrs_host_inflow.h) for
// tests/test_host_inflow_cpu.py: one command per line on stdin, one answer per line on stdout.  Doubles travel as C99 hex floats (or
// nan / inf), so nothing is rounded on the way; integers as decimals.  Built by the test with the host compiler, plain and under the
// sanitizers.
//   slot SLOT                                                   -> rc ...
//   emitter SHAPE ENABLED c(3) d(3) he(2) speed spacing MAXP mass rho
//                                                               -> e s SITES d(3) e1(3) e2(3) | rc ...   (success sets the current emitter)
//   sites                                                       -> ij i j i j ...   (the current emitter's sites through inflow_site)
//   step dt ROOM                                                -> l COUNT ROOM EMITTED DROPPED acc off...   (inflow_schedule on the current emitter)
//   origin off                                                  -> o x y z
//   pos PRECISION off I J                                       -> p x y z   (inflow_origin, inflow_site_pos)
//   block HASLATTICE o(3) sp(3) DX DY DZ HASVEL v(3) N CAP       -> nodes M | rc ...
//   sinks FLAGS NBOXES INTERVAL RESERVED GIVEN box(6 * GIVEN)    -> rc ...   (success sets the current sinks)
//   nosinks                                                     -> rc 0     (no current sinks)
//   refusal SLAB MID IISPH DRIVEN                               -> rc ...
//   slabrefuse                                                  -> rc ...
//   due K INTERVAL                                              -> due 0|1
//   caught PRECISION wo(3) GX GY GZ cs(3) x y z                 -> c 0|1 lo(3) hi(3)   (current sinks; wo, cs and x rounded to the precision first)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "nrs_host_inflow.h"

namespace nrs {
thread_local std::string g_err;
}
using namespace nrs;

static void answer(int rc)
{
    if (rc == NRS_OK) printf("rc 0\n");
    else printf("rc %d %s\n", rc, g_err.c_str());
}
static double num(std::istringstream &in)
{
    std::string t;
    in >> t;
    return strtod(t.c_str(), nullptr); // (hex floats, nan, inf)
}
static uint64_t u64(std::istringstream &in)
{
    std::string t;
    in >> t;
    return strtoull(t.c_str(), nullptr, 10);
}
static long long i64(std::istringstream &in)
{
    std::string t;
    in >> t;
    return strtoll(t.c_str(), nullptr, 10);
}

template <typename R> static void run_pos(const EmitterSlot &sl, double off, int32_t i, int32_t j)
{
    double o[3];
    R x[3];
    inflow_origin(sl, off, o);
    inflow_site_pos<R>(o, sl.f.e1, sl.f.e2, sl.s, i, j, x);
    printf("p %a %a %a\n", (double)x[0], (double)x[1], (double)x[2]);
}
template <typename R> static void run_caught(const nrs_sink_config *c, std::istringstream &in)
{
    R wo[3], cs[3], x[3];
    uint32_t gs[3];
    for (int a = 0; a < 3; ++a) wo[a] = (R)num(in);
    for (int a = 0; a < 3; ++a) gs[a] = (uint32_t)u64(in);
    for (int a = 0; a < 3; ++a) cs[a] = (R)num(in);
    for (int a = 0; a < 3; ++a) x[a] = (R)num(in);
    const CullBounds<R> B = inflow_bounds<R>(c, wo, gs, cs);
    printf("c %d %a %a %a %a %a %a\n", inflow_caught<R>(B, x[0], x[1], x[2]) ? 1 : 0, (double)B.lo[0], (double)B.lo[1], (double)B.lo[2], (double)B.hi[0],
           (double)B.hi[1], (double)B.hi[2]);
}

int main()
{
    EmitterSlot cur;
    nrs_sink_config sinks;
    bool haveSinks = false;
    std::memset(&sinks, 0, sizeof(sinks));
    std::string ln;
    while (std::getline(std::cin, ln)) {
        std::istringstream in(ln);
        std::string cmd;
        in >> cmd;
        if (cmd == "slot") {
            answer(inflow_check_slot((uint32_t)u64(in)));
        } else if (cmd == "emitter") {
            nrs_emitter e;
            std::memset(&e, 0, sizeof(e));
            e.shape = (uint32_t)u64(in); e.enabled = (uint32_t)u64(in);
            for (int a = 0; a < 3; ++a) e.center[a] = num(in);
            for (int a = 0; a < 3; ++a) e.direction[a] = num(in);
            e.half_extent[0] = num(in); e.half_extent[1] = num(in);
            e.speed = num(in); e.spacing = num(in);
            e.max_particles = u64(in);
            const double mass = num(in), rho = num(in);
            EmitterSlot fresh;
            const int rc = inflow_check_emitter(&e, mass, rho, fresh);
            if (rc != NRS_OK) { answer(rc); continue; }
            cur = std::move(fresh);
            printf("e %a %llu", cur.s, (unsigned long long)cur.sites.sites);
            for (int a = 0; a < 3; ++a) printf(" %a", cur.f.d[a]);
            for (int a = 0; a < 3; ++a) printf(" %a", cur.f.e1[a]);
            for (int a = 0; a < 3; ++a) printf(" %a", cur.f.e2[a]);
            printf("\n");
        } else if (cmd == "sites") {
            printf("ij");
            const bool disc = cur.e.shape == NRS_EMITTER_DISC;
            for (uint64_t k = 0; k < cur.sites.sites; ++k) {
                int32_t i = 0, j = 0;
                inflow_site((uint32_t)k, cur.sites.ku, cur.sites.kv, disc, cur.sites.half.data(), cur.sites.start.data(), i, j);
                printf(" %d %d", i, j);
            }
            printf("\n");
        } else if (cmd == "step") {
            const double dt = num(in);
            uint64_t room = u64(in);
            std::vector<double> offs;
            inflow_schedule(cur, dt, room, offs);
            printf("l %zu %llu %llu %llu %a", offs.size(), (unsigned long long)room, (unsigned long long)cur.emitted, (unsigned long long)cur.dropped, cur.acc);
            for (double o : offs) printf(" %a", o);
            printf("\n");
        } else if (cmd == "origin") {
            double o[3];
            inflow_origin(cur, num(in), o);
            printf("o %a %a %a\n", o[0], o[1], o[2]);
        } else if (cmd == "pos") {
            const uint64_t prec = u64(in);
            const double off = num(in);
            const int32_t i = (int32_t)i64(in), j = (int32_t)i64(in);
            if (prec == 64) run_pos<double>(cur, off, i, j); else run_pos<float>(cur, off, i, j);
        } else if (cmd == "block") {
            nrs_lattice L;
            std::memset(&L, 0, sizeof(L));
            const bool hasL = u64(in) != 0;
            for (int a = 0; a < 3; ++a) L.origin[a] = num(in);
            for (int a = 0; a < 3; ++a) L.spacing[a] = num(in);
            for (int a = 0; a < 3; ++a) L.dims[a] = (uint32_t)u64(in);
            const bool hasV = u64(in) != 0;
            double v[3];
            for (int a = 0; a < 3; ++a) v[a] = num(in);
            const uint64_t n = u64(in), cap = u64(in);
            uint64_t m = 0;
            const int rc = inflow_check_block(hasL ? &L : nullptr, hasV ? v : nullptr, n, cap, &m);
            if (rc != NRS_OK) answer(rc);
            else printf("nodes %llu\n", (unsigned long long)m);
        } else if (cmd == "sinks") {
            nrs_sink_config c;
            std::memset(&c, 0, sizeof(c));
            c.flags = (uint32_t)u64(in); c.nboxes = (uint32_t)u64(in); c.interval = (uint32_t)u64(in); c.reserved = (uint32_t)u64(in);
            const uint64_t given = u64(in);
            for (uint64_t b = 0; b < given && b < (uint64_t)NRS_MAX_SINK_BOXES; ++b)
                for (int a = 0; a < 6; ++a) c.boxes[b][a] = num(in);
            const int rc = inflow_check_sinks(&c);
            if (rc == NRS_OK) { sinks = c; haveSinks = true; }
            answer(rc);
        } else if (cmd == "nosinks") {
            haveSinks = false;
            answer(NRS_OK);
        } else if (cmd == "refusal") {
            const bool slab = u64(in) != 0, mid = u64(in) != 0, iisph = u64(in) != 0, driven = u64(in) != 0;
            answer(inflow_refusal(slab, mid, iisph, driven));
        } else if (cmd == "slabrefuse") {
            answer(inflow_refuse_slab());
        } else if (cmd == "due") {
            const uint64_t k = u64(in);
            printf("due %d\n", inflow_cull_due(k, (uint32_t)u64(in)) ? 1 : 0);
        } else if (cmd == "caught") {
            const uint64_t prec = u64(in);
            if (prec == 64) run_caught<double>(haveSinks ? &sinks : nullptr, in); else run_caught<float>(haveSinks ? &sinks : nullptr, in);
        } else if (!cmd.empty()) {
            printf("unknown %s\n", cmd.c_str());
        }
    }
    return 0;
}
