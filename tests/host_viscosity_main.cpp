// host_viscosity_main.cpp — stand-alone driver of the implicit viscosity solve's HIP-free parts (nrs_host_viscosity.h) for
// tests/test_host_viscosity_cpu.py: one command per line on stdin, one answer per line on stdout.  Doubles travel as C99 hex floats
// (or nan / inf), integers as decimals.  Built by the test with the host compiler, plain and under the sanitizers.
//   set NU NUB TOL MIN MAX MOVING   -> set ON NU NUB TOL MIN MAX FIXED CAP | rc ...   (settings kept across lines; unchanged after a refusal)
//   measure RR BB                   -> m VALUE      (the exit test stops on VALUE <= 0; with the settings of the last accepted set)
//   slot ITERATION                  -> slot S
//   sizes CAPACITY REALBYTES        -> sizes VEC DOTS SCALARS
//   alpha RR PQ | beta RRNEW RR     -> v VALUE
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "nrs_host_viscosity.h"

namespace nrs {
thread_local std::string g_err;
}
using namespace nrs;

static double num(std::istringstream &in)
{
    std::string t;
    in >> t;
    return strtod(t.c_str(), nullptr);
}
static uint64_t u64(std::istringstream &in)
{
    std::string t;
    in >> t;
    return strtoull(t.c_str(), nullptr, 10);
}

int main()
{
    ViscSettings s;
    std::string ln;
    while (std::getline(std::cin, ln)) {
        std::istringstream in(ln);
        std::string cmd;
        in >> cmd;
        if (cmd == "set") {
            const double nu = num(in), nuB = num(in), tol = num(in);
            const uint32_t mn = (uint32_t)u64(in), mx = (uint32_t)u64(in);
            const bool moving = u64(in) != 0;
            const int rc = s.set(nu, nuB, tol, mn, mx, moving);
            if (rc != NRS_OK) printf("rc %d %s\n", rc, g_err.c_str());
            else printf("set %d %a %a %a %u %u %d %u\n", s.on() ? 1 : 0, s.nu, s.nuB, s.tol, s.minIters, s.maxIters, s.fixed() ? 1 : 0, s.cap());
        } else if (cmd == "measure") {
            const double rr = num(in), bb = num(in);
            printf("m %a\n", s.measure(rr, bb));
        } else if (cmd == "slot") {
            printf("slot %d\n", visc_rr_slot((uint32_t)u64(in)));
        } else if (cmd == "sizes") {
            const uint64_t cap = u64(in);
            const ViscBufferSizes z = visc_buffer_sizes(cap, (size_t)u64(in));
            printf("sizes %zu %zu %zu\n", z.vec, z.dots, z.scalars);
        } else if (cmd == "alpha") {
            const double rr = num(in), pq = num(in);
            printf("v %a\n", visc_alpha(rr, pq));
        } else if (cmd == "beta") {
            const double rn = num(in), rr = num(in);
            printf("v %a\n", visc_beta(rn, rr));
        } else if (!cmd.empty()) {
            printf("unknown %s\n", cmd.c_str());
        }
    }
    return 0;
}
