// host_diffuse_main.cpp — stand-alone driver of the diffuse particles' HIP-free parts (nrs_host_diffuse.h) for
// tests/test_host_diffuse_cpu.py: one command per line on stdin, one answer per line on stdout.  Doubles travel as C99 hex floats (or
// nan / inf), so nothing is rounded on the way; integers as decimals.  Built by the test with the host compiler, plain and under the
// sanitizers.
//   cfg SIZE CAP SEED ta0 ta1 wc0 wc1 k0 k1 kta kwc l0 l1 kb kd SPRAY BUBBLE MAXPER RESERVED   -> rc ...   (sets the current config, checks it)
//   nocfg                                        -> rc ...
//   dt X                                         -> rc ...
//   refusal SLAB MID IISPH gx gy gz cx cy cz h CONFIGURED   -> rc ...
//   fits N MAXPER                                -> rc ...
//   upload HASPOS HASVEL N CAP                   -> rc ...
//   bytes WHICH D N PRECISION                    -> bytes B
//   route CONFIGURED STEPPED N WHICH ALIVE PRECISION   -> bytes B | rc ...
//   hash SEED STEP SLOT DRAW                     -> hash H
//   uniform PRECISION SEED STEP SLOT DRAW        -> u X
//   clamp PRECISION x lo hi                      -> c X
//   births PRECISION rate dt u                   -> n B         (current config)
//   birth PRECISION STEP SLOT K xi(3) vi(3) rV dt   -> b x y z life vx vy vz   (current config)
//   advect PRECISION x(3) v(3) life vt(3) N g(3) dt lo(3) hi(3)   -> a ALIVE KIND x y z life vx vy vz   (current config)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "nrs_host_diffuse.h"

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
template <typename R> static D3<R> vec(std::istringstream &in)
{
    D3<R> v;
    v.x = (R)num(in); v.y = (R)num(in); v.z = (R)num(in);
    return v;
}

template <typename R> static void run_birth(const nrs_diffuse_config &c, std::istringstream &in)
{
    const uint64_t step = u64(in);
    const uint32_t slot = (uint32_t)u64(in), k = (uint32_t)u64(in);
    const D3<R> xi = vec<R>(in), vi = vec<R>(in);
    const R rV = (R)num(in), dt = (R)num(in);
    const DiffuseBirth<R> b = diffuse_birth<R>(diffuse_cfg<R>(c), step, slot, k, xi, vi, rV, dt);
    printf("b %a %a %a %a %a %a %a\n", (double)b.x.x, (double)b.x.y, (double)b.x.z, (double)b.life, (double)b.v.x, (double)b.v.y, (double)b.v.z);
}
template <typename R> static void run_advect(const nrs_diffuse_config &c, std::istringstream &in)
{
    const D3<R> x = vec<R>(in), v = vec<R>(in);
    const R life = (R)num(in);
    const D3<R> vt = vec<R>(in);
    const uint32_t n = (uint32_t)u64(in);
    const D3<R> g = vec<R>(in);
    const R dt = (R)num(in);
    const D3<R> lo = vec<R>(in), hi = vec<R>(in);
    const DiffuseState<R> s = diffuse_advect<R>(diffuse_cfg<R>(c), x, v, life, vt, n, g, dt, lo, hi);
    printf("a %d %u %a %a %a %a %a %a %a\n", s.alive ? 1 : 0, s.kind, (double)s.x.x, (double)s.x.y, (double)s.x.z, (double)s.life, (double)s.v.x,
           (double)s.v.y, (double)s.v.z);
}

int main()
{
    nrs_diffuse_config cfg = {};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string c;
        in >> c;
        if (c == "cfg") {
            cfg.struct_size = (uint32_t)u64(in);
            cfg.capacity = (uint32_t)u64(in);
            cfg.seed = u64(in);
            for (double *p : {&cfg.tau_ta[0], &cfg.tau_ta[1], &cfg.tau_wc[0], &cfg.tau_wc[1], &cfg.tau_k[0], &cfg.tau_k[1], &cfg.k_ta, &cfg.k_wc,
                              &cfg.lifetime[0], &cfg.lifetime[1], &cfg.k_buoyancy, &cfg.k_drag})
                *p = num(in);
            cfg.spray_below = (uint32_t)u64(in);
            cfg.bubble_above = (uint32_t)u64(in);
            cfg.max_per_particle = (uint32_t)u64(in);
            cfg.reserved = (uint32_t)u64(in);
            answer(diffuse_check_config(&cfg));
        } else if (c == "nocfg") {
            answer(diffuse_check_config(nullptr));
        } else if (c == "dt") {
            answer(diffuse_check_dt(num(in)));
        } else if (c == "refusal") {
            SampleFacts f;
            f.slab = u64(in) != 0; f.midStep = u64(in) != 0; f.iisphInProgress = u64(in) != 0;
            for (int a = 0; a < 3; ++a) f.gridSize[a] = (uint32_t)u64(in);
            for (int a = 0; a < 3; ++a) f.cellSize[a] = num(in);
            f.h = num(in);
            answer(diffuse_refusal(f, u64(in) != 0));
        } else if (c == "fits") {
            const uint64_t n = u64(in);
            answer(diffuse_check_births(n, (uint32_t)u64(in)));
        } else if (c == "upload") {
            static const int dummy = 0;
            const void *p = u64(in) ? &dummy : nullptr, *v = u64(in) ? &dummy : nullptr;
            const uint64_t n = u64(in);
            answer(diffuse_check_upload(p, v, n, (uint32_t)u64(in)));
        } else if (c == "bytes") {
            const uint32_t w = (uint32_t)u64(in);
            const uint64_t D = u64(in), N = u64(in);
            printf("bytes %llu\n", (unsigned long long)diffuse_result_bytes(w, D, N, (int)u64(in)));
        } else if (c == "route") {
            DiffuseLast last;
            last.configured = u64(in) != 0; last.stepped = u64(in) != 0; last.N = u64(in);
            const uint32_t w = (uint32_t)u64(in);
            const uint64_t alive = u64(in);
            uint64_t bytes = 0;
            const int rc = diffuse_route_result(last, w, alive, (int)u64(in), &bytes);
            if (rc != NRS_OK) answer(rc);
            else printf("bytes %llu\n", (unsigned long long)bytes);
        } else if (c == "hash") {
            const uint64_t seed = u64(in), step = u64(in);
            const uint32_t slot = (uint32_t)u64(in);
            printf("hash %llu\n", (unsigned long long)diffuse_hash(seed, step, slot, (uint32_t)u64(in)));
        } else if (c == "uniform") {
            const int prec = (int)u64(in);
            const uint64_t seed = u64(in), step = u64(in);
            const uint32_t slot = (uint32_t)u64(in), draw = (uint32_t)u64(in);
            printf("u %a\n", prec == 64 ? diffuse_uniform<double>(seed, step, slot, draw) : (double)diffuse_uniform<float>(seed, step, slot, draw));
        } else if (c == "clamp") {
            const int prec = (int)u64(in);
            const double x = num(in), lo = num(in), hi = num(in);
            printf("c %a\n", prec == 64 ? diffuse_clamp<double>(x, lo, hi) : (double)diffuse_clamp<float>((float)x, (float)lo, (float)hi));
        } else if (c == "births") {
            const int prec = (int)u64(in);
            const double rate = num(in), dt = num(in), u = num(in);
            printf("n %u\n", prec == 64 ? diffuse_births<double>(diffuse_cfg<double>(cfg), rate, dt, u)
                                         : diffuse_births<float>(diffuse_cfg<float>(cfg), (float)rate, (float)dt, (float)u));
        } else if (c == "birth") {
            if ((int)u64(in) == 64) run_birth<double>(cfg, in);
            else run_birth<float>(cfg, in);
        } else if (c == "advect") {
            if ((int)u64(in) == 64) run_advect<double>(cfg, in);
            else run_advect<float>(cfg, in);
        } else if (!c.empty()) {
            fprintf(stderr, "host_diffuse_main: unknown command %s\n", c.c_str());
            return 2;
        }
    }
    return 0;
}
