// sph_boundary_particles/ss.h — box sampler with the call signature main.cpp:545 uses, and a sampler of triangle meshes.
//
// The reference takes this from the git submodule external/sph_boundary_particles, which is NOT vendored
// (empty directory, commit unknown): its exact sampling pattern is unknown, so this is our own sampler
// behind the same signature — PARITY UNPINNED at this boundary.  The solver itself
// is insensitive to how boundary particles were produced: they are plain input arrays.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "common.h"
#include "nereus_hip.h"

namespace sample_spheres {
namespace ss {

// Samples the six faces of the axis-aligned box [origin, origin+size] with one layer of particles on a
// regular lattice of pitch `radius` (the value main.cpp passes is the particle radius, 0.02); points on
// shared edges/corners are emitted once.  Appends xyz1 to `out`.
inline void sampleBox(std::vector<SVec4> &out, SVec3 origin, SVec3 size, double radius)
{
    const long nx = std::lround(size.x / radius), ny = std::lround(size.y / radius), nz = std::lround(size.z / radius);
    auto emit = [&](long i, long j, long k) {
        out.push_back(make_SVec4((SReal)(origin.x + i * radius), (SReal)(origin.y + j * radius),
                                 (SReal)(origin.z + k * radius), (SReal)1.0));
    };
    for (long i = 0; i <= nx; ++i)
        for (long k = 0; k <= nz; ++k) { emit(i, 0, k); emit(i, ny, k); }
    for (long j = 1; j < ny; ++j)
        for (long k = 0; k <= nz; ++k) { emit(0, j, k); emit(nx, j, k); }
    for (long i = 1; i < nx; ++i)
        for (long j = 1; j < ny; ++j) { emit(i, j, 0); emit(i, j, nz); }
}

// The lattice of pitch `radius` that covers the bounding box [lo, hi] of `vertices` (3 doubles each) plus one node on every side:
// origin[a] = lo[a] - radius, dims[a] = floor((hi[a] - lo[a]) / radius) + 3 (double arithmetic).  Shared by sampleMesh and the callers of
// Nereus::SPH::emitMesh, so that walls and fluid sampled from meshes of one scene sit on lattices of one rule.  No vertices: all zeros.
inline nrs_lattice meshLattice(const std::vector<double> &vertices, double radius)
{
    nrs_lattice L;
    std::memset(&L, 0, sizeof(L));
    if (vertices.size() < 3) return L;
    for (int a = 0; a < 3; ++a) {
        double lo = vertices[a], hi = vertices[a];
        for (size_t i = a; i < vertices.size(); i += 3) { lo = std::min(lo, vertices[i]); hi = std::max(hi, vertices[i]); }
        const double d = std::floor((hi - lo) / radius) + 3.0;
        L.origin[a] = lo - radius;
        L.spacing[a] = radius;
        L.dims[a] = d >= 1.0 && d <= 2147483648.0 ? (uint32_t)d : 0u; // (0 is refused by the library: a lattice too fine to count)
    }
    return L;
}

// Samples a triangle mesh (vertices: 3 doubles each; triangles: 3 indices each, wound counter-clockwise seen from outside) with one
// layer of particles ON its surface: the nodes of meshLattice(vertices, radius) within radius / 2 of the mesh, on either side, each
// moved to its closest point on the mesh (nrs_mesh_particles with NRS_MESH_INSIDE | NRS_MESH_OUTSIDE | NRS_MESH_SNAP, dmin 0,
// dmax radius / 2; on the device).  Points may coincide along sharp edges; getVbi shares the volume between them.  Appends xyz1 to
// `out`; like getVbi it is fatal on error.  Our own sampler: the reference's library samples meshes too, by a pattern that is not known.
inline void sampleMesh(std::vector<SVec4> &out, const std::vector<double> &vertices, const std::vector<uint32_t> &triangles, double radius)
{
    const nrs_mesh mesh = {vertices.data(), (uint64_t)(vertices.size() / 3), triangles.data(), (uint64_t)(triangles.size() / 3)};
    const nrs_lattice L = meshLattice(vertices, radius);
    const nrs_mesh_rule rule = {NRS_MESH_INSIDE | NRS_MESH_OUTSIDE | NRS_MESH_SNAP, 0u, 0.0, radius / 2};
    const int precision = (int)(8 * sizeof(SReal));
    uint64_t count = 0;
    int rc = nrs_mesh_particles(-1, precision, &mesh, &L, &rule, nullptr, 0, &count);
    const size_t at = out.size();
    if (rc == 0 && count) {
        out.resize(at + (size_t)count);
        rc = nrs_mesh_particles(-1, precision, &mesh, &L, &rule, out.data() + at, count, &count);
    }
    if (rc != 0) {
        std::fprintf(stderr, "sampleMesh: nrs_mesh_particles failed (%d): %s\n", rc, nrs_last_error());
        std::exit(EXIT_FAILURE);
    }
}

} // namespace ss
} // namespace sample_spheres
