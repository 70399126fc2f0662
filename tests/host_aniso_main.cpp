// host_aniso_main.cpp — stand-alone driver of the HIP-free host decisions and of the per-particle finishing routine of the anisotropic
// surface reconstruction (nrs_host_aniso.h) for tests/test_host_aniso_cpu.py: one command per line on stdin, one answer per line on
// stdout.  Doubles travel as C99 hex floats (or nan / inf), so nothing is rounded on the way; integers as decimals.  Built by the test
// with the host compiler, plain and under the sanitizers.
//   config NULLP support lambda k_r k_n n_eps reserved h  -> rc ... | cfg support lambda k_r k_n n_eps    (NULLP 1: cfg == NULL)
//   refuse MID IISPH SLAB gx gy gz cx cy cz h             -> rc ...
//   extract iso flags                                     -> rc ... | fields F   (the NRS_FIELD_* flags pass B writes)
//   bytes WHICH N PRECISION                               -> bytes N
//   last ANY N | result WHICH PRECISION                   -> ok | rc ... | bytes N
//   finish PREC h support lambda k_r k_n n_eps  x y z  count sw mx my mz sxx sxy sxz syy syz szz D
//                                                         -> rec cx cy cz bound g00 g01 g02 g11 g12 g22 weight a1 a2 a3
//   cloud PREC h support lambda k_r k_n n_eps  n  x0 y0 z0 x1 ...   (the record of particle 0 among the n, candidates in the order given)
//                                                         -> rec ... count
//   eigen PREC a00 a01 a02 a11 a12 a22                    -> eig l0 l1 l2 u00 u01 u02 u10 u11 u12 u20 u21 u22
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "nrs_host_aniso.h"

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
static AnisoConfig read_config(std::istringstream &in)
{
    AnisoConfig c;
    c.h = num(in); c.support = num(in); c.lambda = num(in); c.k_r = num(in); c.k_n = num(in); c.n_eps = (uint32_t)num(in);
    return c;
}
template <typename R> static void print_record(const AnisoRecord<R> &A)
{
    printf("rec %a %a %a %a %a %a %a %a %a %a %a %a %a %a", (double)A.cx, (double)A.cy, (double)A.cz, (double)A.bound, (double)A.g00, (double)A.g01,
           (double)A.g02, (double)A.g11, (double)A.g12, (double)A.g22, (double)A.weight, (double)A.a1, (double)A.a2, (double)A.a3);
}
template <typename R> static void do_finish(std::istringstream &in)
{
    const AnisoConsts<R> K = aniso_consts<R>(read_config(in));
    const R x = (R)num(in), y = (R)num(in), z = (R)num(in);
    AnisoSums<R> S;
    S.count = (uint32_t)num(in);
    S.sw = (R)num(in);
    S.mx = (R)num(in); S.my = (R)num(in); S.mz = (R)num(in);
    S.sxx = (R)num(in); S.sxy = (R)num(in); S.sxz = (R)num(in); S.syy = (R)num(in); S.syz = (R)num(in); S.szz = (R)num(in);
    S.D = (R)num(in);
    print_record<R>(aniso_finish<R>(K, x, y, z, S));
    printf("\n");
}
template <typename R> static void do_cloud(std::istringstream &in)
{
    const AnisoConsts<R> K = aniso_consts<R>(read_config(in));
    const size_t n = (size_t)num(in);
    std::vector<R> p(3 * n);
    for (size_t i = 0; i < 3 * n; ++i) p[i] = (R)num(in);
    AnisoSums<R> S = aniso_sums_zero<R>();
    for (size_t j = 0; j < n; ++j) aniso_add_neighbour<R>(K, S, p[3 * j] - p[0], p[3 * j + 1] - p[1], p[3 * j + 2] - p[2]);
    print_record<R>(aniso_finish<R>(K, p[0], p[1], p[2], S));
    printf(" %u\n", S.count);
}
template <typename R> static void do_eigen(std::istringstream &in)
{
    const R a00 = (R)num(in), a01 = (R)num(in), a02 = (R)num(in), a11 = (R)num(in), a12 = (R)num(in), a22 = (R)num(in);
    const AnisoEigen<R> E = aniso_eigen<R>(a00, a01, a02, a11, a12, a22);
    printf("eig %a %a %a %a %a %a %a %a %a %a %a %a\n", (double)E.l0, (double)E.l1, (double)E.l2, (double)E.u00, (double)E.u01, (double)E.u02, (double)E.u10,
           (double)E.u11, (double)E.u12, (double)E.u20, (double)E.u21, (double)E.u22);
}

int main()
{
    AnisoLast last;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string c;
        in >> c;
        if (c == "config") {
            const bool null = num(in) != 0;
            nrs_aniso_config g;
            g.support = num(in); g.lambda = num(in); g.k_r = num(in); g.k_n = num(in); g.n_eps = (uint32_t)num(in); g.reserved = (uint32_t)num(in);
            AnisoConfig o;
            const int rc = aniso_check_config(null ? nullptr : &g, num(in), &o);
            if (rc != NRS_OK) { answer(rc); continue; }
            printf("cfg %a %a %a %a %u\n", o.support, o.lambda, o.k_r, o.k_n, o.n_eps);
        } else if (c == "refuse") {
            SampleFacts f;
            f.midStep = num(in) != 0; f.iisphInProgress = num(in) != 0; f.slab = num(in) != 0;
            for (int a = 0; a < 3; ++a) f.gridSize[a] = (uint32_t)num(in);
            for (int a = 0; a < 3; ++a) f.cellSize[a] = num(in);
            f.h = num(in);
            answer(aniso_refusal(f));
        } else if (c == "extract") {
            const double iso = num(in);
            const uint32_t flags = (uint32_t)num(in);
            const int rc = aniso_check_extract(iso, flags);
            if (rc != NRS_OK) { answer(rc); continue; }
            printf("fields %u\n", aniso_sample_fields(flags));
        } else if (c == "bytes") {
            const uint32_t w = (uint32_t)num(in);
            const uint64_t n = (uint64_t)num(in);
            printf("bytes %llu\n", (unsigned long long)aniso_result_bytes(w, n, (int)num(in)));
        } else if (c == "last") {
            last.any = num(in) != 0;
            last.n = (uint64_t)num(in);
            printf("ok\n");
        } else if (c == "result") {
            const uint32_t w = (uint32_t)num(in);
            uint64_t bytes = 0;
            const int rc = aniso_route_result(last, w, (int)num(in), &bytes);
            if (rc != NRS_OK) answer(rc);
            else printf("bytes %llu\n", (unsigned long long)bytes);
        } else if (c == "finish" || c == "cloud" || c == "eigen") {
            const bool dbl = (int)num(in) == 64;
            if (c == "finish") dbl ? do_finish<double>(in) : do_finish<float>(in);
            else if (c == "cloud") dbl ? do_cloud<double>(in) : do_cloud<float>(in);
            else dbl ? do_eigen<double>(in) : do_eigen<float>(in);
        } else if (!c.empty()) {
            fprintf(stderr, "host_aniso_main: unknown command %s\n", c.c_str());
            return 2;
        }
    }
    return 0;
}
