// host_parts_main.cpp — stand-alone driver of the library's HIP-free host components (nrs_host_bodies.h, nrs_host_settings.h,
// nrs_host_slab.h) for tests/test_host_parts_cpu.py: one command per line on stdin, one answer per line on stdout.  Doubles travel as C99 hex floats (or
// nan / inf), so nothing is rounded on the way.  Built by the test with the host compiler, plain and under the sanitizers.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "nrs_host_bodies.h"
#include "nrs_host_settings.h"
#include "nrs_host_slab.h"

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
        } else {
            fprintf(stderr, "host_parts_main: unknown command '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
