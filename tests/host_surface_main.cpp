// host_surface_main.cpp — stand-alone driver of the surface extraction's HIP-free parts (nrs_host_surface.h) for
// tests/test_host_surface_cpu.py: one command per line on stdin, one answer per line on stdout (mesh: several).  Doubles travel as C99
// hex floats (or nan / inf), so nothing is rounded on the way; integers as decimals.  Built by the test with the host compiler, plain
// and under the sanitizers.
//   call ISO FLAGS                               -> rc ...
//   lattice ox oy oz sx sy sz dx dy dz           -> rc ... | nodes N
//   nolattice                                    -> rc ...
//   fields FLAGS                                 -> fields F                (the NRS_FIELD_* flags of the extract's sample call)
//   bytes WHICH V T PRECISION                    -> bytes N
//   last ANY FLAGS V T | result WHICH PRECISION  -> ok | rc ... | bytes N
//   drop                                         -> ok                      (nrs_surface_release)
//   mesh PRECISION ox oy oz sx sy sz dx dy dz ISO f0 f1 ...   (the nodes' densities in linear order)
//        -> mesh V T, then V lines "v x y z t", then T lines "t a b c": the per-node and per-cell routines of the kernels, driven
//           serially in the kernels' order (count, scan, vertices, triangles)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "nrs_host_surface.h"

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
static void read_lattice(std::istringstream &in, nrs_lattice &L)
{
    for (int a = 0; a < 3; ++a) L.origin[a] = num(in);
    for (int a = 0; a < 3; ++a) L.spacing[a] = num(in);
    for (int a = 0; a < 3; ++a) L.dims[a] = (uint32_t)num(in);
    L.reserved = 0;
}

template <typename R> static int mesh(const nrs_lattice &lat, double isoD, std::istringstream &in)
{
    uint64_t nodes64 = 0;
    const int rc = surface_check_lattice(&lat, &nodes64);
    if (rc != NRS_OK) { answer(rc); return 0; }
    const Lattice L = lattice_from(lat);
    const uint32_t nodes = (uint32_t)nodes64, nx = L.dims[0], ny = L.dims[1];
    std::vector<R> dens(nodes);
    for (uint32_t q = 0; q < nodes; ++q) dens[q] = (R)num(in);
    if (!in) { fprintf(stderr, "host_surface_main: mesh: too few densities\n"); return 2; }
    const R iso = (R)isoD;
    auto offset = [&](uint32_t d) { return (d & 1u) + ((d >> 1) & 1u) * nx + ((d >> 2) & 1u) * nx * ny; };
    auto load = [&](uint32_t q, uint32_t have, R f[8]) {
        for (uint32_t d = 0; d < 8; ++d) f[d] = (d & ~have) ? (R)0 : dens[q + offset(d)];
    };
    // count and scan
    std::vector<uint32_t> nodeOff(nodes), nodeMask(nodes), cellOff(nodes), cellBits(nodes);
    uint32_t V = 0, T = 0;
    for (uint32_t q = 0; q < nodes; ++q) {
        const uint32_t i = q % nx, j = (q / nx) % ny, k = q / nx / ny, have = surf_have(L, i, j, k);
        R f[8];
        load(q, have, f);
        uint32_t count = 0;
        nodeMask[q] = surf_node_edges<R>(f, iso, have, &count);
        nodeOff[q] = V;
        V += count;
        cellBits[q] = have == 7u ? surf_inside_bits<R>(f, iso, have) : 0u;
        cellOff[q] = T;
        T += have == 7u ? surf_cell_count(cellBits[q]) : 0u;
    }
    printf("mesh %u %u\n", V, T);
    // vertices
    uint32_t v = 0;
    for (uint32_t q = 0; q < nodes; ++q) {
        const uint32_t idx[3] = {q % nx, (q / nx) % ny, q / nx / ny};
        for (uint32_t e = 0; e < 7; ++e) {
            if (!((nodeMask[q] >> e) & 1u)) continue;
            const uint32_t d = surf_edge_dir(e);
            const R t = surf_vertex_t<R>(iso, dens[q], dens[q + offset(d)]);
            printf("v");
            for (int a = 0; a < 3; ++a) {
                const R p0 = surf_node_coord<R>(L, a, idx[a]), p1 = ((d >> a) & 1u) ? surf_node_coord<R>(L, a, idx[a] + 1u) : p0;
                printf(" %a", (double)surf_lerp<R>(p0, p1, t));
            }
            printf(" %a\n", (double)t);
            if (v++ != nodeOff[q] + surf_popcount(nodeMask[q] & ((1u << e) - 1u))) { fprintf(stderr, "host_surface_main: vertex numbering\n"); return 2; }
        }
    }
    // triangles
    std::vector<uint32_t> tri(3 * (size_t)T);
    for (uint32_t q = 0; q < nodes; ++q) {
        if (!cellBits[q]) continue;
        const uint32_t n = surf_cell_triangles(cellBits[q], [&](uint32_t k, uint32_t c0, uint32_t e0, uint32_t c1, uint32_t e1, uint32_t c2, uint32_t e2) {
            const uint32_t cs[3] = {c0, c1, c2}, es[3] = {e0, e1, e2};
            for (int i = 0; i < 3; ++i) {
                const uint32_t nq = q + offset(cs[i]);
                tri.at(3 * (size_t)(cellOff[q] + k) + i) = nodeOff[nq] + surf_popcount(nodeMask[nq] & ((1u << es[i]) - 1u));
            }
        });
        if (n != surf_cell_count(cellBits[q])) { fprintf(stderr, "host_surface_main: cell count\n"); return 2; }
    }
    for (uint32_t k = 0; k < T; ++k) printf("t %u %u %u\n", tri[3 * k], tri[3 * k + 1], tri[3 * k + 2]);
    return 0;
}

int main()
{
    SurfaceLast last;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string c;
        in >> c;
        if (c == "call") {
            const double iso = num(in);
            answer(surface_check_call(iso, (uint32_t)num(in)));
        } else if (c == "lattice") {
            nrs_lattice L;
            read_lattice(in, L);
            uint64_t nodes = 0;
            const int rc = surface_check_lattice(&L, &nodes);
            if (rc != NRS_OK) { answer(rc); continue; }
            printf("nodes %llu\n", (unsigned long long)nodes);
        } else if (c == "nolattice") {
            answer(surface_check_lattice(nullptr, nullptr));
        } else if (c == "fields") {
            printf("fields %u\n", surface_sample_fields((uint32_t)num(in)));
        } else if (c == "bytes") {
            const uint32_t w = (uint32_t)num(in);
            const uint64_t V = (uint64_t)num(in), T = (uint64_t)num(in);
            printf("bytes %llu\n", (unsigned long long)surface_result_bytes(w, V, T, (int)num(in)));
        } else if (c == "drop") {
            last = SurfaceLast();
            printf("ok\n");
        } else if (c == "last") {
            last.any = num(in) != 0;
            last.flags = (uint32_t)num(in);
            last.V = (uint64_t)num(in);
            last.T = (uint64_t)num(in);
            printf("ok\n");
        } else if (c == "result") {
            const uint32_t w = (uint32_t)num(in);
            uint64_t bytes = 0;
            const int rc = surface_route_result(last, w, (int)num(in), &bytes);
            if (rc != NRS_OK) answer(rc);
            else printf("bytes %llu\n", (unsigned long long)bytes);
        } else if (c == "mesh") {
            const int precision = (int)num(in);
            nrs_lattice L;
            read_lattice(in, L);
            const double iso = num(in);
            const int rc = precision == 64 ? mesh<double>(L, iso, in) : mesh<float>(L, iso, in);
            if (rc) return rc;
        } else if (!c.empty()) {
            fprintf(stderr, "host_surface_main: unknown command %s\n", c.c_str());
            return 2;
        }
    }
    return 0;
}
