// host_track_main.cpp — stand-alone driver of particle tracking's HIP-free parts (nrs_host_track.h) for tests/test_host_track_cpu.py:
// one command per line on stdin, one answer per line on stdout.  Doubles travel as C99 hex floats (or nan / inf), integers as decimals.
// Built by the test with the host compiler, plain and under the sanitizers.
//   flags F                                          -> rc ...
//   slabenable | slabconfigure                       -> rc ...
//   refusal ON FLAGS MID IISPH NEEDATTR SETTLED      -> rc ...
//   birth STEPS                                      -> b BIRTH
//   next N                                           -> rc 0      (sets the id counter)
//   reserve COUNT                                    -> ids FIRST NEXT | rc ...   (the counter is unchanged after a refusal)
//   uploaded COUNT id...                             -> next NEXT | rc ...        (likewise)
//   freshupload N FIRST COUNT | freshsetn N NN       -> f FIRST COUNT
//   upload WHICH FLAGS HASSRC FIRST COUNT N          -> rc ...
//   route WHICH FLAGS HAVELOCATE N LOCATED PRECISION -> bytes B | rc ...
//   emitvalue SLOT HASA                              -> rc ...
//   locate FIRST COUNT                               -> rc ...
//   diffuse HASK k(4) dt                             -> rc ...
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "nrs_host_track.h"

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
    return strtod(t.c_str(), nullptr);
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

int main()
{
    TrackIds ids;
    std::string ln;
    while (std::getline(std::cin, ln)) {
        std::istringstream in(ln);
        std::string cmd;
        in >> cmd;
        if (cmd == "flags") {
            answer(track_check_flags((uint32_t)u64(in)));
        } else if (cmd == "slabenable") {
            answer(track_refuse_slab());
        } else if (cmd == "slabconfigure") {
            answer(track_refuse_slab_configure());
        } else if (cmd == "refusal") {
            TrackFacts f;
            f.on = u64(in) != 0; f.flags = (uint32_t)u64(in); f.midStep = u64(in) != 0; f.iisphInProgress = u64(in) != 0;
            const bool needAttr = u64(in) != 0, settled = u64(in) != 0;
            answer(track_refusal(f, needAttr, settled));
        } else if (cmd == "birth") {
            printf("b %u\n", track_birth(u64(in)));
        } else if (cmd == "next") {
            ids.next = u64(in);
            answer(NRS_OK);
        } else if (cmd == "reserve") {
            uint32_t first = 0;
            const int rc = ids.reserve(u64(in), &first);
            if (rc != NRS_OK) answer(rc);
            else printf("ids %u %llu\n", first, (unsigned long long)ids.next);
        } else if (cmd == "uploaded") {
            const uint64_t count = u64(in);
            std::vector<uint32_t> src(count);
            for (uint64_t i = 0; i < count; ++i) src[i] = (uint32_t)u64(in);
            uint64_t next = ids.next;
            const int rc = track_ids_uploaded(src.data(), count, next, &next);
            if (rc != NRS_OK) { answer(rc); continue; }
            ids.next = next;
            printf("next %llu\n", (unsigned long long)ids.next);
        } else if (cmd == "freshupload") {
            const uint64_t n = u64(in), first = u64(in), count = u64(in);
            const TrackFresh f = track_fresh_after_upload(n, first, count);
            printf("f %llu %llu\n", (unsigned long long)f.first, (unsigned long long)f.count);
        } else if (cmd == "freshsetn") {
            const uint64_t n = u64(in), nn = u64(in);
            const TrackFresh f = track_fresh_after_set_n(n, nn);
            printf("f %llu %llu\n", (unsigned long long)f.first, (unsigned long long)f.count);
        } else if (cmd == "upload") {
            const uint32_t which = (uint32_t)u64(in), flags = (uint32_t)u64(in);
            const bool has = u64(in) != 0;
            const uint64_t first = u64(in), count = u64(in), n = u64(in);
            uint32_t word = 0;
            answer(track_check_upload(which, flags, has ? &word : nullptr, first, count, n));
        } else if (cmd == "route") {
            const uint32_t which = (uint32_t)u64(in), flags = (uint32_t)u64(in);
            const bool have = u64(in) != 0;
            const uint64_t n = u64(in), located = u64(in);
            const int prec = (int)u64(in);
            uint64_t bytes = 0;
            const int rc = track_route_result(which, flags, have, n, located, prec, &bytes);
            if (rc != NRS_OK) answer(rc);
            else printf("bytes %llu\n", (unsigned long long)bytes);
        } else if (cmd == "emitvalue") {
            const int32_t slot = (int32_t)i64(in);
            const double a[4] = {0.0, 0.0, 0.0, 0.0};
            answer(track_check_emit_value(slot, u64(in) ? a : nullptr));
        } else if (cmd == "locate") {
            const uint64_t first = u64(in), count = u64(in);
            answer(track_check_locate(first, count));
        } else if (cmd == "diffuse") {
            const bool has = u64(in) != 0;
            double k[4];
            for (int c = 0; c < 4; ++c) k[c] = num(in);
            const double dt = num(in);
            answer(track_check_diffuse(has ? k : nullptr, dt));
        } else if (!cmd.empty()) {
            printf("unknown %s\n", cmd.c_str());
        }
    }
    return 0;
}
