// host_mesh_main.cpp — stand-alone driver of the mesh sampling's HIP-free parts (nrs_host_mesh.h) for tests/test_host_mesh_cpu.py:
// one command per line on stdin, one answer per line on stdout.  Doubles travel as C99 hex floats (or nan / inf), so nothing is
// rounded on the way; integers as decimals.  Built by the test with the host compiler, plain and under the sanitizers.
//   mesh HASMESH NV NT GV v(3 * GV) GT t(3 * GT)   -> rc ...   (nv = NV, nt = NT as claimed; GV / GT triples given, 0: a NULL array;
//                                                               success sets the current mesh)
//   gather                                         -> g x ...  (mesh_gather of the current mesh: 9 doubles per triangle)
//   rule HASRULE FLAGS RESERVED dmin dmax          -> r USEW USED dmin2 dmax2 | rc ...
//   precision P                                    -> rc ...
//   snap                                           -> rc ...   (nrs_emit_mesh's refusal)
//   plan N                                         -> plan B first count first count ...
//   sel FLAGS dmin dmax w d2                       -> s 0|1    (mesh_selected under mesh_select_from)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "nrs_host_mesh.h"

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

int main()
{
    std::vector<double> verts;
    std::vector<uint32_t> tris;
    nrs_mesh cur = {nullptr, 0, nullptr, 0};
    std::string ln;
    while (std::getline(std::cin, ln)) {
        std::istringstream in(ln);
        std::string cmd;
        in >> cmd;
        if (cmd == "mesh") {
            const bool has = u64(in) != 0;
            nrs_mesh m;
            m.nv = u64(in);
            m.nt = u64(in);
            std::vector<double> v(3 * (size_t)u64(in));
            for (double &x : v) x = num(in);
            std::vector<uint32_t> t(3 * (size_t)u64(in));
            for (uint32_t &x : t) x = (uint32_t)u64(in);
            m.vertices = v.empty() ? nullptr : v.data();
            m.triangles = t.empty() ? nullptr : t.data();
            const int rc = mesh_check_mesh(has ? &m : nullptr);
            if (rc == NRS_OK) {
                verts.swap(v);
                tris.swap(t);
                cur = m; // (the swapped vectors keep their storage)
            }
            answer(rc);
        } else if (cmd == "gather") {
            std::vector<double> tri9;
            if (cur.nt) mesh_gather(cur, tri9);
            printf("g");
            for (double x : tri9) printf(" %a", x);
            printf("\n");
        } else if (cmd == "rule") {
            const bool has = u64(in) != 0;
            nrs_mesh_rule r;
            r.flags = (uint32_t)u64(in);
            r.reserved = (uint32_t)u64(in);
            r.dmin = num(in);
            r.dmax = num(in);
            const int rc = mesh_check_rule(has ? &r : nullptr);
            if (rc != NRS_OK) { answer(rc); continue; }
            const MeshSelect s = mesh_select_from(r);
            printf("r %u %u %a %a\n", s.useW, s.useD, s.dmin2, s.dmax2);
        } else if (cmd == "precision") {
            answer(mesh_check_precision((int)(long long)u64(in)));
        } else if (cmd == "snap") {
            answer(mesh_refuse_snap());
        } else if (cmd == "plan") {
            const uint64_t n = u64(in), nb = mesh_batches(n);
            printf("plan %llu", (unsigned long long)nb);
            for (uint64_t b = 0; b < nb; ++b) {
                uint64_t first;
                uint32_t count;
                mesh_batch(n, b, first, count);
                printf(" %llu %u", (unsigned long long)first, count);
            }
            printf("\n");
        } else if (cmd == "sel") {
            nrs_mesh_rule r;
            r.flags = (uint32_t)u64(in);
            r.reserved = 0;
            r.dmin = num(in);
            r.dmax = num(in);
            const double w = num(in), d2 = num(in);
            printf("s %d\n", mesh_selected(mesh_select_from(r), w, d2) ? 1 : 0);
        } else {
            printf("unknown %s\n", cmd.c_str());
        }
    }
    return 0;
}
