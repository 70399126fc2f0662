// host_sample_main.cpp — stand-alone driver of the field sampler's HIP-free host decisions (nrs_host_sample.h) for
// tests/test_host_sample_cpu.py: one command per line on stdin, one answer per line on stdout.  Doubles travel as C99 hex floats (or
// nan / inf), so nothing is rounded on the way; integers as decimals.  Built by the test with the host compiler, plain and under the
// sanitizers.
//   fields F                                   -> rc ...
//   points NULLP M                             -> rc ...                 (NULLP 1: points4 == NULL)
//   lattice ox oy oz sx sy sz dx dy dz         -> rc ... | nodes N
//   bytes FIELD M PRECISION                    -> bytes N
//   refuse MID IISPH SLAB gx gy gz cx cy cz h  -> rc ...
//   cache  S P G B                             -> build 0|1 builds N     (asks needs_build for the key, builds if so)
//   drop                                       -> ok                     (nrs_sample_release)
//   last ANY FIELDS M | result FIELD PRECISION -> ok | rc ... | bytes N
//   builds                                     -> builds N               (nrs_sample_builds)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "nrs_host_sample.h"

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

int main()
{
    SampleCache cache;
    SampleLast last;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string c;
        in >> c;
        if (c == "fields") {
            answer(sample_check_fields((uint32_t)num(in)));
        } else if (c == "points") {
            static const char dummy[16] = {0};
            const bool null = num(in) != 0;
            answer(sample_check_points(null ? nullptr : dummy, (uint64_t)num(in)));
        } else if (c == "lattice") {
            nrs_lattice L;
            for (int a = 0; a < 3; ++a) L.origin[a] = num(in);
            for (int a = 0; a < 3; ++a) L.spacing[a] = num(in);
            for (int a = 0; a < 3; ++a) L.dims[a] = (uint32_t)num(in);
            L.reserved = 0;
            uint64_t nodes = 0;
            const int rc = sample_check_lattice(&L, &nodes);
            if (rc != NRS_OK) { answer(rc); continue; }
            printf("nodes %llu\n", (unsigned long long)nodes);
        } else if (c == "nolattice") {
            answer(sample_check_lattice(nullptr, nullptr));
        } else if (c == "bytes") {
            const uint32_t f = (uint32_t)num(in);
            const uint64_t m = (uint64_t)num(in);
            printf("bytes %llu\n", (unsigned long long)sample_result_bytes(f, m, (int)num(in)));
        } else if (c == "refuse") {
            SampleFacts f;
            f.midStep = num(in) != 0; f.iisphInProgress = num(in) != 0; f.slab = num(in) != 0;
            for (int a = 0; a < 3; ++a) f.gridSize[a] = (uint32_t)num(in);
            for (int a = 0; a < 3; ++a) f.cellSize[a] = num(in);
            f.h = num(in);
            answer(sample_refusal(f));
        } else if (c == "cache") {
            SampleKey k;
            k.stepsDone = (uint64_t)num(in); k.particleGen = (uint64_t)num(in); k.gridGen = (uint64_t)num(in); k.boundaryGen = (uint64_t)num(in);
            const bool b = cache.needs_build(k);
            if (b) cache.built(k);
            printf("build %d builds %llu\n", b ? 1 : 0, (unsigned long long)cache.builds);
        } else if (c == "drop") {
            cache.dropped();
            last = SampleLast();
            printf("ok\n");
        } else if (c == "last") {
            last.any = num(in) != 0;
            last.fields = (uint32_t)num(in);
            last.m = (uint64_t)num(in);
            printf("ok\n");
        } else if (c == "result") {
            const uint32_t f = (uint32_t)num(in);
            uint64_t bytes = 0;
            const int rc = sample_route_result(last, f, (int)num(in), &bytes);
            if (rc != NRS_OK) answer(rc);
            else printf("bytes %llu\n", (unsigned long long)bytes);
        } else if (c == "builds") {
            printf("builds %llu\n", (unsigned long long)cache.builds);
        } else if (!c.empty()) {
            fprintf(stderr, "host_sample_main: unknown command %s\n", c.c_str());
            return 2;
        }
    }
    return 0;
}
